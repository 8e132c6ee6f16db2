"""The sizes the field backward's callers allocate by, pinned on the CPU (no device call): the dE
workspace (csrc/field_de_ws.h states its layout; the formula here is written out independently of
it), the split passes' stash and the MLP pass's grid sizes."""
import pytest

from ncnerf_amd import _lib

NS = [0, 1, 3, 4, 5, 15, 16, 17, 32767, 32768, 32769, 65536, 8192 * 64, 2 ** 31]


def dE_floats(n):
    """header (4) + [16][e] packed pairs + 4 classes x 3 coordinates x e rounded up to whole units of
    32768 samples + 32 queue words, e = n rounded up to 4."""
    if n <= 0:
        return 0
    e = (n + 3) & ~3
    return 4 + 16 * e + 4 * 3 * ((e + 32767) // 32768) * 32768 + 32


def bwd_blocks(n):
    """one workgroup per 32 groups of 16 samples, between 1 and 256"""
    groups = (n + 15) // 16
    return min(256, max(1, (groups + 31) // 32))


@pytest.mark.parametrize("n", NS + [-1])
def test_dE_workspace_floats(n):
    assert _lib.lib().ncn_field_bwd_dE_floats(n) == dE_floats(n)


@pytest.mark.parametrize("n", NS + [-1])
def test_stash_floats(n):
    # per group of 16 samples: 64 lanes x 4 two-byte operands (128 floats) + 16 fp32 row-0 elements
    assert _lib.lib().ncn_field_bwd_stash_floats(n) == (144 * ((n + 15) // 16) if n > 0 else 0)


@pytest.mark.parametrize("n", NS)
def test_mlp_pass_blocks(n):
    L = _lib.lib()
    nb = bwd_blocks(n)
    assert L.ncn_field_bwd_blocks(n) == nb
    # the sigma pass (part 2) runs two workgroups per CU: twice the grid, at most 512
    assert [L.ncn_field_bwd_part_blocks(n, part) for part in (1, 2, 3)] == [nb, min(512, 2 * nb), nb]
