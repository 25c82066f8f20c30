"""Bit plans of the head-group codecs (FMT_GRP / FMT_GRPR rows): how many bits every 64-channel group of a boundary
gets, allocated from the channel-group relevance / sensitivity tables of the relevance pass.  The wire format only
carries a plan (``wire.with_plan``); nothing here touches a message."""
from __future__ import annotations

import torch

from .wire import GROUP_BITS


def boundary_group_relevance(table, boundary: int, groups: int) -> list:
    """The channel-group relevance of the tensor crossing the boundary after layer ``boundary`` from a
    [layers][groups] table of the relevance ENTERING each layer (``channel_group_relevance.json``): row
    ``boundary + 1``.  After the last layer the tensor is the final norm's input, which the table does not hold;
    its last row (the stream entering the last layer) stands in.  No table: every group equal.  A dict table
    ``{"relevance": ..., "sensitivity": ...}`` (``load_group_tables``) gives its relevance."""
    if isinstance(table, dict):
        table = table.get("relevance")
    if table is None:
        return [1.0] * groups
    t = torch.as_tensor(table, dtype=torch.float32)
    return [float(v) for v in t[min(boundary + 1, t.shape[0] - 1)]]


def boundary_group_plan(table, boundary: int, groups: int, avg_bits: float = 4.0) -> tuple:
    """The bit plan of the head-group codec at the boundary after layer ``boundary``.

    ``table`` = ``{"relevance": [layers][G], "sensitivity": [layers][G]}`` (``load_group_tables``): the MSE
    allocation over the groups' quantization sensitivity when it is there (``allocate_group_bits(model="mse")``),
    else the first-order allocation over the LRP relevance (``model="linear"``, the round-3 allocator); a plain
    [layers][G] list is a relevance table; None: the uniform plan (every group at ``avg_bits`` when that is a
    width, else the MSE allocation of equal weights: the nearest widths, as evenly as the budget allows)."""
    if table is None:
        return allocate_group_bits([1.0] * groups, avg_bits, model="mse")
    if isinstance(table, dict) and table.get("sensitivity") is not None:
        w = boundary_group_relevance({"relevance": table["sensitivity"]}, boundary, groups)
        return allocate_group_bits(w, avg_bits, model="mse")
    return allocate_group_bits(boundary_group_relevance(table, boundary, groups), avg_bits, model="linear")


def _qmax(bits: int) -> int:
    return (1 << (bits - 1)) - 1


def allocate_group_bits(weights, avg_bits: float = 4.0, model: str = "mse", widths=GROUP_BITS) -> tuple:
    """Bit allocation over the 64-channel groups of a boundary: every group starts at the narrowest width and the
    budget ``avg_bits * G`` bits goes, one step up the width ladder at a time, to the step with the largest error
    reduction per bit.  Error models of a group g quantized at b bits (max-abs scale, step amax / qmax_b):

    * ``"mse"``: the expected squared first-order output change, W_g / (12 qmax_b^2) with W_g the group's
      quantization sensitivity sum_t max_c |x_tc|^2 sum_c dx_tc^2 (``ops.reference.group_sens``: a rounding error
      uniform in +-step/2 per channel, independent across channels, propagated through the gradient dx).  The
      error falls 4-9x per added bit, so a group gets a wider code only where its sensitivity is that much larger
      than the others' - the outlier-heavy groups;
    * ``"linear"``: R_g / qmax_b with R_g the LRP relevance sum |x dx| (the round-3 allocator: error ~ sum |dx|
      step / 2), only on the widths 2 / 4 / 8.

    The error reductions per bit fall along the ladder (convex), so the greedy allocation is optimal for the
    model.  Equal weights give the uniform plan."""
    w = [max(float(r), 0.0) for r in weights]
    G = len(w)
    if not any(w):
        w = [1.0] * G
    if model == "linear":
        ladder = (2, 4, 8)
        err = {b: 1.0 / _qmax(b) for b in ladder}
    elif model == "mse":
        ladder = tuple(sorted(widths))
        err = {b: 1.0 / _qmax(b) ** 2 for b in ladder}
    else:
        raise ValueError(f"unknown allocation model {model!r} (mse | linear)")
    nxt = {ladder[i]: ladder[i + 1] for i in range(len(ladder) - 1)}
    bits = [ladder[0]] * G
    budget = int(round(avg_bits * G)) - ladder[0] * G
    while budget > 0:
        best, best_gain = -1, 0.0
        for g in range(G):
            b = bits[g]
            if b not in nxt:
                continue
            nb = nxt[b]
            cost = nb - b
            if cost > budget:
                continue
            gain = w[g] * (err[b] - err[nb]) / cost
            if gain > best_gain or (gain == best_gain and best >= 0 and w[g] > w[best]):
                best, best_gain = g, gain
        if best < 0:
            break
        budget -= nxt[bits[best]] - bits[best]
        bits[best] = nxt[bits[best]]
    return tuple(bits)


def load_group_tables(relevance_path: str):
    """``channel_group_relevance.json`` and, when the relevance pass wrote it beside, the sensitivity table
    ``channel_group_sensitivity.json`` -> {"relevance": tensor, "sensitivity": tensor or None}."""
    import json
    import os
    with open(relevance_path) as f:
        rel = torch.tensor(json.load(f), dtype=torch.float32)
    sp = os.path.join(os.path.dirname(os.path.abspath(relevance_path)), "channel_group_sensitivity.json")
    sens = None
    if os.path.exists(sp):
        with open(sp) as f:
            sens = torch.tensor(json.load(f), dtype=torch.float32)
    return {"relevance": rel, "sensitivity": sens}
