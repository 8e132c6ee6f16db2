"""Host restatement of the reference's SemanticMetrics (metrics/semantic_metrics.py) in plain torch:
torchmetrics is not needed.  update() follows semantic_metrics.py:23-40 (argmax, mask, confusion
matrix), compute() semantic_metrics.py:42-66 line for line in float32, as the reference.

torchmetrics' confusion_matrix(preds, target, num_classes=K) of label vectors is
bincount(target * K + preds, minlength=K * K).reshape(K, K): rows the target, columns the prediction.
"""
import math

import torch

KEYS = ("miou", "miou_valid_cls", "total_acc", "cls_avg_acc")


def update(conf, pred_logits, target_labels, ignore_label=-1):
    """semantic_metrics.py:23-40 -> (conf + this call's matrix, counted, out of range, pred_labels).
    conf (K, K) int64; pred_logits (n, K); target_labels (n), already shifted.  A label outside
    [0, K) that is not ignore_label is left out and counted (torchmetrics would refuse it)."""
    K = conf.shape[0]
    assert pred_logits.dim() == 2 and target_labels.dim() == 1
    pred = torch.argmax(pred_logits, dim=1)           # :30
    t = target_labels.long()
    keep = t != ignore_label                          # :31
    inside = (t >= 0) & (t < K)
    out_of_range = int((keep & ~inside).sum())
    keep &= inside
    counted = int(keep.sum())
    if counted:                                       # :33-40
        conf = conf + torch.bincount(t[keep] * K + pred[keep], minlength=K * K).reshape(K, K)
    return conf, counted, out_of_range, pred


def compute(conf):
    """The scores of semantic_metrics.py:42-66 from conf (K, K) int64, each operation in float32 and in
    the reference's order (the line numbers are the reference's)."""
    K = conf.shape[0]
    rows = conf.float().sum(dim=1)
    share = conf / rows[:, None]                      # :43  each row over its sum: NaN rows where it is 0
    present = ~torch.isnan(share.sum(1))              # :46-47  the classes the ground truth holds
    cls_avg_acc = torch.nanmean(share.diagonal())     # :49
    total_acc = conf.diagonal().sum() / conf.sum()    # :50  integer / integer -> float32
    ious = torch.zeros(K)
    for c in range(K):                                # :52-55
        ious[c] = conf[c, c] / (conf[c, :].sum() + conf[:, c].sum() - conf[c, c])
    miou = torch.nanmean(ious)                        # :56
    miou_valid_cls = ious[present].mean()             # :57
    return {"miou": miou.item(), "miou_valid_cls": miou_valid_cls.item(), "total_acc": total_acc.item(),
            "cls_avg_acc": cls_avg_acc.item(), "ious": ious.tolist()}


def same(a, b, rel):
    """Both NaN, or |a - b| <= rel * |b|."""
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rel * abs(b)


def make_case(n, K, seed, void_share=0.2):
    """Random logits (n, K) float32 and RAW labels (n) int64 in 0..K, 0 = void (about void_share)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, K, generator=g)
    labels = torch.randint(1, K + 1, (n,), generator=g)
    labels[torch.rand(n, generator=g) < void_share] = 0
    return logits, labels
