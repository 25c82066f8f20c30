"""Loader for the in-tree gfx950 kernel library ``_native/libedge_kernels.so``.

The library is plain HIP C ABI (no torch headers), built by ``build.py`` with
``hipcc --offload-arch=gfx950``.  Kernels are launched on the current torch
stream, so they compose with torch ops, CUDA-graph capture and RCCL streams.

On a GPU process the library is mandatory: ``lib()`` raises instead of silently
falling back to the PyTorch reference path.
"""
from __future__ import annotations

import ctypes
import os

import torch

from ..utils import poison as _poison

_HERE = os.path.dirname(os.path.abspath(__file__))
# EDGE_KERNEL_LIB: load another build of the library (A/B of two kernel builds in one GPU session)
LIB_PATH = os.environ.get("EDGE_KERNEL_LIB") or os.path.join(os.path.dirname(_HERE), "_native", "libedge_kernels.so")

_lib = None

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_f = ctypes.c_float
c_ll = ctypes.c_longlong

_SIGS = {
    "edge_rmsnorm": [c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_p],
    "edge_layernorm": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_p],
    "edge_embedding": [c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    "edge_gemm": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_p, c_p],
    "edge_row_ssq": [c_p, c_p, c_i, c_i, c_p],
    "edge_row_rscale": [c_p, c_p, c_i, c_i, c_i, c_f, c_p],
    "edge_gemm_set_tile": [c_i],
    "edge_gemm_set_ring": [c_i],
    "edge_gemm_set_store_wait": [c_i],
    "edge_gemm_ssq_parts": [c_i, c_i, c_i, c_i, c_i, c_i],
    "edge_gemm_qkv_rope": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p, c_p,
                           c_i, c_f, c_p],
    "edge_gemm_lse": [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p],
    "edge_lse_reduce": [c_p, c_p, c_p, c_p, c_i, c_i, c_p],
    "edge_flash_attn_fwd": [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p],
    "edge_attn_lastrow": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "edge_attn_colsum": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "edge_head_combine": [c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_f, c_p],
    "edge_select": [c_p, c_i, c_i, c_i, c_p, c_ll, c_i, c_f, c_ll, c_p],
    "edge_set_mask": [c_p, c_ll, c_i, c_i, c_i, c_p],
    "edge_channel_stats": [c_p, c_p, c_ll, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p],
    "edge_rowmax": [c_p, c_p, c_i, c_i, c_p],
    "edge_pack": [c_p, c_p, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i,
                  c_i, c_p],
    "edge_lrp_attn_bwd": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "edge_lrp_rope_pack": [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p],
    "edge_swiglu_il": [c_p, c_p, c_ll, c_i, c_p],
    "edge_lrp_swiglu_bwd": [c_p, c_p, c_p, c_ll, c_i, c_p],
    "edge_lrp_gelu_bwd": [c_p, c_p, c_ll, c_p],
    "edge_lrp_ln_bwd": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p],
    "edge_ln_rstd": [c_p, c_p, c_i, c_i, c_f, c_p],
    "edge_unpack": [c_p, c_p, c_ll, c_ll, c_ll, c_ll, c_ll, c_ll, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i,
                    c_i, c_i, c_p],
    # fp32 execution mode (h3 split-fp16 GEMM operands, fp32 attention / norms / codec)
    "edge_rmsnorm_f32_rstd": [c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_f, c_p, c_p],
    "edge_gemm_swiglu_raw": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p],
    "edge_gemm_f32_swiglu_raw": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_f, c_f, c_p],
    "edge_gemm_f32_cs": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_p, c_f,
                         c_p, c_p, c_p, c_p, c_f, c_p],
    "edge_lrp_attn_bwd_h3": [c_p] * 12 + [c_i] * 5 + [c_f] * 3 + [c_p],
    "edge_gemm_f32_lrp_swiglu": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p],
    "edge_gemm_f32_np_ok": [c_i, c_i, c_i],
    "edge_gemm_f32_np": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_f, c_p, c_p, c_f, c_f, c_p, c_p,
                         c_p, c_p],
    "edge_row_rscale_mul": [c_p, c_p, c_p, c_i, c_i, c_i, c_f, c_p],
    "edge_gemm_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_f, c_f, c_p],
    "edge_gemm_qkv_rope_f32": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f,
                               c_f, c_p, c_p, c_f, c_f, c_p, c_p],
    "edge_flash_attn_fwd_h3p": [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_p, c_p],
    "edge_flash_attn_fwd_f32": [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_p],
    "edge_attn_lastrow_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_f, c_p],
    "edge_attn_colsum_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_f, c_p],
    "edge_rmsnorm_f32": [c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_f, c_p],
    "edge_layernorm_f32": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_f, c_f, c_f, c_p],
    "edge_split_h3": [c_p, c_p, c_p, c_i, c_i, c_f, c_p],
    "edge_embedding_f32": [c_p, c_p, c_p, c_i, c_i, c_i, c_p],
    # fp32 AttnLRP backward (csrc/lrp_f32.hip)
    "edge_lrp_rope_pack_h3": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p],
    "edge_lrp_rope_pack_h3_gs": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p],
    "edge_split_h3_dyn": [c_p, c_p, c_p, c_p, c_i, c_i, c_p],
    "edge_lrp_swiglu_bwd_h3": [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p],
    "edge_lrp_gelu_bwd_h3": [c_p, c_p, c_p, c_p, c_i, c_i, c_p],
    "edge_act_h3": [c_p, c_p, c_ll, c_i, c_i, c_f, c_p],
    "edge_row_rstd_f32": [c_p, c_p, c_i, c_i, c_f, c_i, c_p],
    "edge_lrp_ln_bwd_f32": [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p],
    "edge_group_absprod": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    # measured quantization error of the head groups (csrc/codec.hip): the kernel, and the row chunks its workspace has
    "edge_group_quant_err": [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p],
    "edge_group_quant_err_chunks": [c_i],
    # debug (csrc/debug.hip): LDS + register-file poison before every kernel under EDGE_POISON=2
    "edge_poison_lds": [c_p],
    "edge_poison_lds_bytes": [],
}


_LL_RESULT = {"edge_gemm_ws_floats"}


class NativeLibraryMissing(RuntimeError):
    pass


def tuning() -> bool:
    """Test hooks (EDGE_BENCH_FAIL_RANK) are honoured only with EDGE_TUNING=1, so a stray environment variable can
    never change a production run."""
    return os.environ.get("EDGE_TUNING", "0") not in ("", "0")


def available() -> bool:
    return os.path.exists(LIB_PATH)


def lib():
    """Return the loaded ctypes library, loading it on first use (raises if absent)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryMissing(
                f"{LIB_PATH} not found: build the gfx950 kernels first "
                "(python -c 'import __graft_entry__ as g; g.build()')")
        L = ctypes.CDLL(LIB_PATH)
        for name, argt in _SIGS.items():
            if os.environ.get("EDGE_KERNEL_LIB") and not hasattr(L, name):
                continue  # an older build under A/B: entry points it predates stay unbound
            fn = getattr(L, name)
            fn.argtypes = argt
            fn.restype = c_ll if name in _LL_RESULT else c_i
        _lib = L
    return _lib


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


_NO_LAUNCH = {"edge_gemm_set_tile", "edge_gemm_set_ring", "edge_gemm_set_store_wait", "edge_gemm_ssq_parts", "edge_poison_lds", "edge_poison_lds_bytes",
              "edge_gemm_f32_np_ok", "edge_group_quant_err_chunks"}


def call(name: str, *args) -> None:
    if _poison.level() >= 2 and name not in _NO_LAUNCH:
        # EDGE_POISON=2: every LDS byte and register of the chip is all-ones (NaN) when this kernel starts
        rc = lib().edge_poison_lds(stream())
        if rc != 0:
            raise RuntimeError(f"edge_poison_lds failed with HIP error {rc}")
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed with HIP error {rc}")
