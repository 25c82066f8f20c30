"""The cases of test_codec_edges.py (ties, saturation, zero units, Hadamard rows, the ends of the exponent range, NaN
and Inf) on the HIP kernels of csrc/codec.hip: GPU message bytes against the CPU oracle's, GPU decode against the CPU
decode, and both against the independent fp64 / enumerated-grid references of that module."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import test_codec_digests as D
import test_codec_edges as E
from llm_inference_in_distributed_edge_networks_amd import codec as C
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


@lru_cache(maxsize=None)
def cpu_ref(builder, *key):
    """(case, CPU message, layout, CPU fp32 decode); shared by the tests, never modified."""
    case = builder(*key)
    return (case, *case.cpu())


def gpu_run(case):
    msg, L = C.encode(case.x.to(DEV), case.spec, case.B, case.S, case.ratio, case.imp.to(DEV))
    return msg, L, C.decode(msg, case.spec, L, F32).cpu()


def agree(builder, key, check):
    """GPU bytes == CPU bytes, GPU decode == CPU decode, and the GPU's message and decode pass the independent check;
    bf16 activations: the decode into bf16 is the CPU's fp32 decode rounded to bf16."""
    case, m_cpu, L, y_cpu = cpu_ref(builder, *key)
    m_dev, L2, y_gpu = gpu_run(case)
    assert L2 == L
    m_gpu = m_dev.cpu()
    assert torch.equal(m_gpu, m_cpu), f"{(m_gpu != m_cpu).sum().item()} bytes differ"
    assert torch.equal(y_gpu, y_cpu), f"{(y_gpu != y_cpu).sum().item()} decoded values differ"
    check(case, m_gpu, L, y_gpu)
    if case.x.dtype == BF16:
        assert torch.equal(C.decode(m_dev, case.spec, L, BF16).cpu(), y_cpu.to(BF16))
    return case, m_dev, L


@pytest.mark.parametrize("name,ratio,B,S,H", E.tie_params())
def test_ties(name, ratio, B, S, H):
    agree(E.tie_case, (name, ratio, B, S, H), E.check_ties)


@pytest.mark.parametrize("name,ratio", [("int8_token", 0.0), ("mixed_int4_int8", 0.5), ("mixed_int2_int8", 0.5),
                                        ("int8_token_keep", 0.5), ("mixed_rgroup_int8", 0.5), ("rgroup", 0.0)])
def test_ties_bf16(name, ratio):
    agree(E.tie_case, (name, ratio, 3, 37, 576, BF16), E.check_ties)


@pytest.mark.parametrize("name,ratio,variant,B,S,H", E.formula_params())
def test_formulas(name, ratio, variant, B, S, H):
    agree(E.formula_case, (name, ratio, variant, B, S, H), E.check_formula)


@pytest.mark.parametrize("name,ratio", [("ref_int4_global", 0.5), ("channel_8", 0.0), ("channel_1_max", 0.0)])
@pytest.mark.parametrize("variant", list(E.FORMULA_MAXIMA))
def test_formulas_bf16(name, ratio, variant):
    agree(E.formula_case, (name, ratio, variant, 3, 37, 576, BF16), E.check_formula)


@pytest.mark.parametrize("variant", list(E.FORMULA_MAXIMA))
def test_window_code_minus8_decodes(variant):
    """The int4 code -8 of the window mode, which no input encodes to (see minus8_message): decoded as the CPU does."""
    case = E.formula_case("ref_int4_global", 0.5, variant, 3, 64, 128)
    msg, L, rows = E.minus8_message(case)
    y = C.decode(msg.to(DEV), case.spec, L, F32).cpu()
    assert torch.equal(y, C.decode(msg, case.spec, L, F32))
    E.check_minus8(case, y, rows)


@pytest.mark.parametrize("name,ratio,B,S,H", E.mx_params())
def test_mx_grids(name, ratio, B, S, H):
    agree(E.mx_case, (name, ratio, B, S, H), E.check_mx)


@pytest.mark.parametrize("name,ratio", [("mxfp4", 0.0), ("mxfp8", 0.0), ("mixed_mxfp4_mxfp8", 0.5)])
def test_mx_grids_bf16(name, ratio):
    agree(E.mx_case, (name, ratio, 3, 37, 96, BF16), E.check_mx)


@pytest.mark.parametrize("B,S,H", E.ZERO_SHAPES)
@pytest.mark.parametrize("variant", ["units", "all"])
@pytest.mark.parametrize("name", sorted(set(E.ZERO_CODECS) - {"channel_1_mean"}))   # its mean: summation order
def test_zero_units(name, variant, B, S, H):
    agree(E.zero_case, (name, B, S, H, variant), E.check_zeros)


@pytest.mark.parametrize("B,S,H", E.ROT_SHAPES)
@pytest.mark.parametrize("kind", E.ROT_PLANS)
def test_hadamard_rows(kind, B, S, H):
    agree(E.rot_case, (kind, B, S, H), E.check_rot)


@pytest.mark.parametrize("B,S,H", E.BOUND_SHAPES)
@pytest.mark.parametrize("name", E.BOUND_CODECS)
def test_rounding_bound(name, B, S, H):
    agree(E.bound_case, (name, B, S, H), E.check_bound)


@pytest.mark.parametrize("B,S,H", E.ENDS_SHAPES)
@pytest.mark.parametrize("variant", ["normal", "tiny"])
@pytest.mark.parametrize("name", E.BOUND_CODECS)
def test_exponent_ends(name, variant, B, S, H):
    """Windows in the normal regime (3e38 - 2^120 where the format itself overflows earlier -, and 2^-120 for the
    integer and head-group formats, whose int8 scale is already a denormal): GPU bytes == CPU bytes, GPU decode ==
    CPU decode, and check_bound on the GPU's result.  Windows below 2^-100 (MX at 2^-120, every format at 2^-126 and
    1e-39): finite and bounded on the GPU as on the CPU; whether the bytes agree there is printed, not asserted.

    Recorded on an MI355X (every codec of BOUND_CODECS, both shapes): in all of those windows - max-abs 2^-126 and
    the denormal 1e-39 for every format, 2^-120 for the MX formats - the GPU's message bytes and its decode were
    identical to the CPU's.  The scaled converts, the divides and the multiplies keep fp32 denormals (inputs, scales
    and results) exactly as the CPU arithmetic does; nothing was flushed."""
    case, m_cpu, L, y_cpu = cpu_ref(E.ends_case, name, variant, B, S, H)
    m_dev, L2, y_gpu = gpu_run(case)
    assert L2 == L
    m_gpu = m_dev.cpu()
    strict = E.check_ends(case, m_gpu, L, y_gpu)
    rest = np.ones(L.total, dtype=bool)
    for b in range(B):
        wb = E.window_bytes(L, case.spec, b)
        rest &= ~wb
        same_bytes = bool(np.array_equal(m_gpu.numpy()[wb], m_cpu.numpy()[wb]))
        rows = slice(b * S, b * S + S)
        same_dec = bool(torch.equal(y_gpu[rows], y_cpu[rows]))
        print(f"EDGE-ENDS {name} H={H} S={S} max|x|={case.info['M'][b]:.4g} strict={b in strict} "
              f"bytes_equal={same_bytes} decode_equal={same_dec} "
              f"bytes_differ={int((m_gpu.numpy()[wb] != m_cpu.numpy()[wb]).sum())}")
        if b in strict:
            assert same_bytes and same_dec, (name, b)
    assert np.array_equal(m_gpu.numpy()[rest], m_cpu.numpy()[rest])      # header, mask, plan, padding


@pytest.mark.parametrize("B,S,H", E.NONFINITE_SHAPES)
@pytest.mark.parametrize("placement", E.PLACEMENTS)
@pytest.mark.parametrize("name", E.NONFINITE_CODECS)
def test_nonfinite(name, placement, B, S, H):
    """(a) the NaN and the Inf decode non-finite - from the GPU's own message, from the CPU's message decoded on the
    GPU and from the GPU's message decoded on the CPU; (b) outside window 0 the GPU's bytes are the CPU's and the
    decode is that of the clean tensor.  channel_1_mean (a channel mean: summation order) only (a)."""
    case, m_cpu, L, y_cpu = cpu_ref(E.nonfinite_case, name, placement, B, S, H)
    m_clean, y_clean = E.clean_cpu(name, placement, B, S, H)
    m_dev, L2, y_gpu = gpu_run(case)
    assert L2 == L
    m_gpu = m_dev.cpu()
    if name == "channel_1_mean":
        for r, c in case.info["pos"]:
            assert not torch.isfinite(y_gpu[r, c])
        assert torch.isfinite(y_gpu[S:]).all()
        return
    for y in (y_gpu, C.decode(m_cpu.to(DEV), case.spec, L, F32).cpu(), C.decode(m_gpu, case.spec, L, F32)):
        E.check_nonfinite(case, m_gpu, L, y, y_clean)
    w0 = E.window_bytes(L, case.spec, 0)
    assert np.array_equal(m_gpu.numpy()[~w0], m_cpu.numpy()[~w0])
    if case.spec.lo_fmt in W.MX_FORMATS or case.spec.hi_fmt in W.MX_FORMATS:
        E.check_mx_nonfinite(case, m_gpu, L, y_gpu, y_clean)


DIGEST_CASES = [c for c in D.cases() if c[3] == "f32" and c[1] != "channel_1_mean"]


@pytest.mark.parametrize("key,name,spec,dn,ratio,sel", DIGEST_CASES, ids=[c[0] for c in DIGEST_CASES])
def test_gpu_digest(key, name, spec, dn, ratio, sel):
    """The GPU's message and fp32 decode of the fp32-activation cases of tests/golden/codec_digests.json: the bytes the
    CPU codec emitted before it and the kernels were restructured together.  channel_1_mean (a channel mean:
    summation order) is not compared."""
    assert D.run_case(spec, dn, ratio, sel, DEV) == D.fixture()[key]
