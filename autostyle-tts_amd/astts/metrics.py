"""Classification metrics of the reference's evaluation (src/evaluate_base_model.py:86, src/ft_llm.py: sklearn's
``f1_score(labels, preds, average="weighted")``), restated so that the product imports no sklearn."""
from __future__ import annotations

from typing import Sequence


def weighted_f1(labels: Sequence, preds: Sequence) -> float:
    """Per-class F1 averaged with the class's share of ``labels`` as weight.  The classes are every value met in ``labels`` OR
    ``preds``: a prediction outside the label set is a class of its own with support 0 -- it adds nothing itself and costs the class it
    was mistaken for a false negative, as in sklearn.  A class with no true positive has F1 0 (sklearn's zero_division default)."""
    if len(labels) != len(preds):
        raise ValueError("weighted_f1: one prediction per label")
    if not len(labels):
        raise ValueError("weighted_f1: no samples")
    total = 0.0
    for c in set(labels) | set(preds):
        tp = sum(1 for l, p in zip(labels, preds) if l == c and p == c)
        support = sum(1 for l in labels if l == c)
        predicted = sum(1 for p in preds if p == c)
        f1 = 2.0 * tp / (support + predicted) if tp else 0.0
        total += f1 * support
    return total / len(labels)
