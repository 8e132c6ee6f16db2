/*
 * ncnerf_sem.h — the semantic side of libncnerf.so's validation and data paths: the confusion matrix
 * and the scores of the reference's SemanticMetrics (metrics/semantic_metrics.py) on the device, and
 * the gather of integer labels from a device-resident plane (the integer counterpart of
 * ncn_batch_labels_fw).  A sixth header beside ncnerf.h, ncnerf_metrics.h, ncnerf_geom.h,
 * ncnerf_mesh.h and ncnerf_heads.h, in the same grammar and under the same rules (ncnerf.h, top):
 * plain device pointers, `void* stream` last, nothing allocated, nothing synchronised, 0 or a
 * hipError_t returned.  THIS FILE IS PARSED by ncnerf_amd/_lib.py exactly as ncnerf.h is, into a
 * table of its own; every entry point here returns int.  (The kernels live in csrc/metrics_sem.h,
 * a stage of metrics.hip, and in loss_geom.hip.)
 *
 * Every count is an integer and is accumulated with integer atomics, which are exact and order
 * free: two calls on the same inputs give the same bits.  No float atomics.
 */
#ifndef NCNERF_SEM_H
#define NCNERF_SEM_H
#include <stdint.h>

#define NCN_SEM_MAX_CLASSES 64

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one view into the confusion matrix, one streaming launch of P(n_pix) = min(ceil(n_pix / 256),
 *      1024) workgroups.  logits is (n_pix, n_cls) f32 with unit channel stride and row_stride >=
 *      n_cls floats between rows (the renderer's `sem` is a channel slice of a wider buffer and is
 *      read in place; what lies between the rows is never read).  labels is (n_pix) int64.
 *      Per pixel i: p = argmax of the row under torch's rule (a NaN beats every number, the first NaN
 *      wins, otherwise the first maximum wins; a row of -inf gives 0); t = labels[i] + label_shift.
 *      t == ignore_label: the pixel is skipped.  0 <= t < n_cls: conf[t * n_cls + p] += 1 (rows are
 *      the target, columns the prediction, as torchmetrics' confusion_matrix) and counts[0] += 1.
 *      Any other t: counts[1] += 1, nothing else (such a label indexes nothing).
 *      conf (n_cls * n_cls) and counts (2) int64 are ADDED INTO: the caller zeroes them once, and one
 *      matrix accumulates over the views.  pred_labels, unless NULL, is (n_pix) int32 and receives p of
 *      EVERY pixel, the skipped ones too.  1 <= n_cls <= NCN_SEM_MAX_CLASSES, n_pix <= 2^40; anything
 *      else is hipErrorInvalidValue and nothing is launched.  n_pix == 0 launches nothing. ---- */
int ncn_sem_confusion(const float* logits, int64_t row_stride, const int64_t* labels, int label_shift,
                      int ignore_label, int64_t n_pix, int n_cls, int64_t* conf, int64_t* counts,
                      int32_t* pred_labels, void* stream);

/* ---- SemanticMetrics.compute() (semantic_metrics.py:42-66) by one workgroup.  out is (4 + n_cls) f32:
 *      miou, miou_valid_cls, total_acc, cls_avg_acc, ious[0 .. n_cls).  With row_c / col_c the sums of
 *      row / column c: iou_c = conf[c][c] / (row_c + col_c - conf[c][c]), NaN at 0 / 0; miou = the mean
 *      of the non-NaN ious (nanmean); miou_valid_cls = the mean of iou_c over the classes with
 *      row_c > 0; total_acc = trace / total; cls_avg_acc = the mean of conf[c][c] / row_c over
 *      row_c > 0; a mean over no class, and 0 / 0, is NaN.  Every quotient and mean is taken in f64
 *      (the classes summed in order) and rounded once to f32. ---- */
int ncn_sem_finalise(const int64_t* conf, int n_cls, float* out, void* stream);

/* ---- integer label gather of a drawn batch: out[r] = plane[img_idxs[r]][pix_idxs[r]] widened to
 *      int64.  plane is (n_images, n_pixels) of uint8, int32 or int64 (plane_bytes 1, 4 or 8; anything
 *      else is hipErrorInvalidValue).  An index outside its range gives 0 (void, which the loss and
 *      the metric ignore), never an out-of-bounds read. ---- */
int ncn_batch_semantics_fw(const int64_t* img_idxs, const int64_t* pix_idxs, int64_t n_rays, const void* plane,
                           int plane_bytes, int n_images, int64_t n_pixels, int64_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
