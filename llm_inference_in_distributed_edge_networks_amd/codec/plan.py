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


GROUP_PLAN_MODES = ("auto", "measured")


def boundary_group_plan(table, boundary: int, groups: int, avg_bits: float = 4.0, *, mode: str = "auto",
                        rot: bool = False) -> tuple:
    """The bit plan of the head-group codec at the boundary after layer ``boundary``.

    ``mode="auto"``: ``table`` = ``{"relevance": [layers][G], "sensitivity": [layers][G]}`` (``load_group_tables``):
    the MSE allocation over the groups' quantization sensitivity when it is there
    (``allocate_group_bits(model="mse")``), else the first-order allocation over the LRP relevance
    (``model="linear"``, the round-3 allocator); a plain [layers][G] list is a relevance table; None: the uniform plan
    (every group at ``avg_bits`` when that is a width, else the MSE allocation of equal weights: the nearest widths,
    as evenly as the budget allows).

    ``mode="measured"``: the exact allocation (``allocate_group_bits_measured``) against the table's measured
    quantization error ``table["quant_error"]`` [layers][G][2][widths]: the row of the stream entering layer
    ``boundary + 1`` (the last row after the last layer, as ``boundary_group_relevance``) in the plain basis, or with
    ``rot`` (the codec's group rows are rotated, ``rgroup_rot``) the Hadamard basis.  No such table is an error."""
    if mode not in GROUP_PLAN_MODES:
        raise ValueError(f"group plan mode must be one of {GROUP_PLAN_MODES}, got {mode!r}")
    if mode == "measured":
        qe = table.get("quant_error") if isinstance(table, dict) else None
        if qe is None:
            raise ValueError("group plan mode 'measured' needs the measured quantization-error table "
                             "(channel_group_quant_error.json beside the relevance table; the relevance pass "
                             "writes it)")
        qe = torch.as_tensor(qe, dtype=torch.float32)
        if qe.dim() != 4 or qe.shape[1] != groups or qe.shape[2] != 2 or qe.shape[3] != len(GROUP_BITS):
            raise ValueError(f"measured quantization-error table is {tuple(qe.shape)}, expected "
                             f"[layers][{groups}][2][{len(GROUP_BITS)}]")
        return allocate_group_bits_measured(qe[min(boundary + 1, qe.shape[0] - 1), :, int(bool(rot))], avg_bits)
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


def plan_cost(err, plan, widths=GROUP_BITS) -> float:
    """sum_g err[g][index of plan[g] in widths]: what a plan costs by a measured table."""
    return float(sum(float(err[g][widths.index(b)]) for g, b in enumerate(plan)))


def allocate_group_bits_measured(err, avg_bits: float = 4.0, min_gain: float = 0.0, widths=GROUP_BITS) -> tuple:
    """The bit plan that minimises a MEASURED error table: ``err`` [G][len(widths)], err[g][j] the error of group g
    quantized at ``widths[j]`` bits (one boundary and basis of ``ops.group_quant_err`` /
    ``channel_group_quant_error.json``).  Returns the exact minimiser of sum_g err[g][b_g] subject to
    sum_g b_g <= round(avg_bits G), by dynamic programming over (group, bits used) - measured errors need not be
    convex along the width ladder, so the greedy of ``allocate_group_bits`` is not used.  Ties go to the smaller
    sum of bits, then to the lexicographically smaller plan.  The uniform plan (``boundary_group_plan(None, ...)``)
    is returned unless cost(best) < (1 - min_gain) cost(uniform): by the table's own measure the result is never worse
    than uniform.  A non-finite or negative entry is an error naming its group."""
    widths = tuple(widths)
    E = [[float(v) for v in row] for row in (err.tolist() if isinstance(err, torch.Tensor) else err)]
    G = len(E)
    for g, row in enumerate(E):
        if len(row) != len(widths):
            raise ValueError(f"measured error table: group {g} has {len(row)} entries for the widths {widths}")
        if any(not (v >= 0.0) or v == float("inf") for v in row):
            raise ValueError(f"measured error table: group {g} has a non-finite or negative entry {row}")
    uniform = allocate_group_bits([1.0] * G, avg_bits, model="mse", widths=widths)
    budget = int(round(avg_bits * G))
    if budget < min(widths) * G:
        return uniform
    # best[u] after g groups: (cost, plan) of the cheapest plan of the first g groups using exactly u bits; at equal
    # cost the lexicographically smaller plan.  Costs are sums in group order, so equal plans compare equal.
    best = {0: (0.0, ())}
    for g in range(G):
        nxt = {}
        for u, (c, pl) in best.items():
            for j, b in enumerate(widths):
                if u + b > budget:
                    continue
                cand = (c + E[g][j], pl + (b,))
                if u + b not in nxt or cand < nxt[u + b]:
                    nxt[u + b] = cand
        best = nxt
    cost, bits_used, plan = min((c, u, pl) for u, (c, pl) in best.items())
    if not cost < (1.0 - min_gain) * plan_cost(E, uniform, widths):
        return uniform
    return plan


def load_group_tables(relevance_path: str):
    """``channel_group_relevance.json`` and, when the relevance pass wrote them beside, the sensitivity table
    ``channel_group_sensitivity.json`` and the measured quantization-error table
    ``channel_group_quant_error.json`` ([layers][G][2 bases][widths]) -> {"relevance": tensor, "sensitivity": tensor
    or None, "quant_error": tensor or None}."""
    import json
    import os
    with open(relevance_path) as f:
        rel = torch.tensor(json.load(f), dtype=torch.float32)
    beside = os.path.dirname(os.path.abspath(relevance_path))
    extra = {}
    for key, name in (("sensitivity", "channel_group_sensitivity.json"),
                      ("quant_error", "channel_group_quant_error.json")):
        extra[key] = None
        if os.path.exists(os.path.join(beside, name)):
            with open(os.path.join(beside, name)) as f:
                extra[key] = torch.tensor(json.load(f), dtype=torch.float32)
    return {"relevance": rel, **extra}
