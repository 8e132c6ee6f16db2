#!/bin/bash
# Diagnostic builds of the whole library with -D sets (comma-separated) -> tools/_build/lib_<name>.so
# The sources are the Makefile's SRCS (+ errors.cpp), so the list cannot fall behind it.
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/_build
PKG=normal-clustering-nerf_amd
SRCS=$(make -s -C $PKG -f Makefile -f <(printf 'print-srcs:\n\t@echo $(SRCS)\n') print-srcs)
for v in "$@"; do
  name=${v//=/_}; name=${name//,/+}
  defs=$(echo "$v" | tr ',' '\n' | sed 's/^/-D/' | tr '\n' ' ')
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -munsafe-fp-atomics $defs \
    $(for s in $SRCS; do echo $PKG/$s; done) $PKG/csrc/errors.cpp -o tools/_build/lib_${name,,}.so &
done
wait
