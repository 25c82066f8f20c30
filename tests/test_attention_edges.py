"""Attention and importance cases for ragged windows and hard softmax rows (tests/helpers.py ``attention_case``), on
the CPU: every case has a finite fp64 reference and the CPU fp32 oracle meets the tolerances the HIP kernels are
held to in test_attention_edges_gpu.py; those tolerances tell the causal attention from one whose mask or tail is
off by one; and the window generator produces the ragged windows the whole-model GPU tests run."""
from functools import lru_cache

import pytest
import torch

import helpers as T
from llm_inference_in_distributed_edge_networks_amd import ops
from llm_inference_in_distributed_edge_networks_amd.eval.data import synthetic_stream
from llm_inference_in_distributed_edge_networks_amd.eval.windows import batches, sliding_windows
from llm_inference_in_distributed_edge_networks_amd.ops import reference as R

LAYOUTS = T.EDGE_LAYOUTS + [T.EDGE_LAYOUT_G16]
OUTPUTS = ("o", "lse", "lastrow", "colsum")


def oracle_outputs(q, k, vt, S):
    """The CPU fp32 oracle path of the ops (what the CPU configuration runs)."""
    o, lse = ops.attention(q, k, vt, S, need_lse=True)
    return {"o": o, "lse": lse, "lastrow": ops.attn_lastrow(q, k, S), "colsum": ops.attn_colsum(q, k, lse, S)}


@lru_cache(maxsize=16)
def edge_ref(kid, layout, S):
    """(q, k, v, V^T, fp64 references {o, lse, lastrow, colsum}, caps, the CPU fp32 oracle's outputs); shared by
    the tests, never modified."""
    q, k, v = T.edge_case(kid, *layout, S)
    vt = T.vt_of(v, S)
    o, lse = R.attention(q.double(), k.double(), vt.double(), S, need_lse=True)
    ref = {"o": o, "lse": lse, "lastrow": R.attn_lastrow(q.double(), k.double(), S),
           "colsum": R.attn_colsum(q.double(), k.double(), lse, S)}
    return q, k, v, vt, ref, T.edge_caps(q, k, v, o, S), oracle_outputs(q, k, vt, S)


@pytest.mark.parametrize("S", T.EDGE_S)
@pytest.mark.parametrize("kid", T.EDGE_KIND_IDS)
def test_cases(kid, S):
    for layout in LAYOUTS:
        q, k, v, vt, ref, caps, got = edge_ref(kid, layout, S)
        assert all(torch.isfinite(r).all() for r in ref.values()), (kid, layout, S)
        # the references are one probability matrix's: the three oracle functions agree with the explicit form
        for name, r in zip(OUTPUTS, T.attention_all64(q, k, v, S)):
            assert T.edge_err(name, r, ref[name]) < 1e-12, (name, layout)
        assert 2.0 ** 15 >= max(R.h3_scale(float(t.abs().max())) * float(t.abs().max()) for t in (q, k, v))
        for name in OUTPUTS:
            err = T.edge_err(name, got[name], ref[name])
            assert err <= caps[name], (name, layout, err, caps[name])


def test_flat_closed_form():
    """q = 0: o_i is the running mean of v and lse_i = log(i + 1) (the reference itself, against the closed form)."""
    S, layout = 129, (3, 4, 2)
    q, k, v, vt, ref, _, _ = edge_ref("flat", layout, S)
    n = torch.arange(1, S + 1, dtype=torch.float64)
    assert torch.allclose(ref["lse"], n.log().expand(3, 4, S), rtol=0, atol=1e-13)
    mean = v.double().cumsum(2) / n.view(1, 1, S, 1)                               # [B, Hkv, S, 64]
    want = mean.repeat_interleave(2, 1).permute(0, 2, 1, 3).reshape(3 * S, 4 * 64)
    assert torch.allclose(ref["o"], want, rtol=0, atol=1e-13)
    assert torch.allclose(ref["colsum"][0, 0], (1 / n).flip(0).cumsum(0).flip(0), rtol=0, atol=1e-13)


# which outputs each wrong mask moves: a mask one key too wide never changes the last row (it sees every key anyway)
MUTANTS = {"mask+1": (dict(shift=1), ("o", "lse", "colsum")),
           "mask-1": (dict(shift=-1), OUTPUTS),
           "pad_last": (dict(pad_last=True), OUTPUTS)}


@pytest.mark.parametrize("S", [s for s in T.EDGE_S if s >= 2])
@pytest.mark.parametrize("kid", ["rand", "flat"])
def test_detection(kid, S):
    """A condition on the cases: the fp32 oracle's outputs FAIL the tolerances against a reference whose causal mask
    is off by one in either direction, or that treats key S - 1 as padding - on every output the mutation touches.
    A tolerance that cannot see an off-by-one tail is not a test."""
    for layout in LAYOUTS:
        q, k, v, vt, ref, caps, got = edge_ref(kid, layout, S)
        for mut, (kw, moved) in MUTANTS.items():
            bad = dict(zip(OUTPUTS, T.attention_all64(q, k, v, S, **kw)))
            for name in moved:
                err = T.edge_err(name, got[name], bad[name])
                assert err > caps[name], (mut, name, layout, err, caps[name])


def test_ragged_windows():
    """The two ragged configurations of the whole-model GPU tests: a stream whose last window is shorter than
    max_length (its own batch), and a stream shorter than max_length (a single window)."""
    toks = synthetic_stream(2997, 512, 4)
    wins = sliding_windows(2997, 256, 32)
    last = wins[-1]
    assert all(w.length == 256 for w in wins[:-1])
    assert (last.length, last.trg_len, last.first_scored, last.end) == (245, 21, 223, 2997)
    bl = list(batches(toks, wins, 4))[-3:]
    assert len(wins) == 87 and [tuple(b.ids.shape) for b in bl] == [(4, 256), (2, 256), (1, 245)]
    rag = bl[-1]
    assert rag.ids.shape == (1, 245) and rag.n_rows.tolist() == [21.0] and rag.weights.tolist() == [20.0]
    assert rag.rows.tolist() == list(range(223, 244))
    assert torch.equal(rag.targets, toks.view(-1)[last.begin + 224:last.begin + 245])
    toks = synthetic_stream(77, 512, 4)
    wins = sliding_windows(77, 256, 32)
    assert len(wins) == 1 and (wins[0].length, wins[0].trg_len, wins[0].first_scored) == (77, 77, 0)
    (b,) = list(batches(toks, wins, 4))
    assert b.ids.shape == (1, 77) and b.n_rows.tolist() == [76.0] and b.weights.tolist() == [76.0]
    assert b.rows.tolist() == list(range(76)) and torch.equal(b.targets, toks.view(-1)[1:77])
