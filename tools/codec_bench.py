"""Pack / unpack time of boundary codecs against each other in one process (device events, alternating repeats).

    python tools/codec_bench.py --codecs rgroup,rgroup_rot --plan-bits 4 --json-out OUT/codec_bench.json
    python tools/codec_bench.py --codecs passthrough,passthrough@bf16,passthrough@fp16,passthrough@fp16s

    python tools/codec_bench.py --codecs mxfp8,mxfp4@e2m3,mxfp4@e3m2,mxfp4
    python tools/codec_bench.py --codecs mxfp4,mxfp4@nvfp4 --hidden 4096

``name@wire`` is codec ``name`` with its activation-dtype rows on the 16-bit wire ``wire`` (``with_native_wire``),
``name@e2m3`` / ``name@e3m2`` with its MXFP4 rows as MXFP6 rows of that element type, ``name@nvfp4`` with them as NVFP4
rows (``with_mx_elem``), ``name@rot``
with its MX rows Hadamard-rotated (``with_mx_rot``), ``name@top8`` with the 8 largest channels of its per-token int
rows kept exact (``with_outliers``), ``name@h128`` / ``name@full`` with those rows Hadamard-rotated per 128-channel block /
as whole rows (``with_row_rot``); modifiers chain: ``mxfp4@e2m3@rot``.

Every codec packs the same activations ([B * S, H], randn with one massive channel) into its own preallocated
message (the pack kernel alone: selection and statistics run once, before) and decodes it into a preallocated
tensor; a repeat times ``--iters`` back-to-back calls of one direction
between two events, and the codecs alternate within every repeat so that clock and neighbour drift hit all alike.
``--fork-variants 10,40`` times something else: the sweep's step between prefix and suffix for V variants of each
codec (V / 10 importance sources x ratios 0.1 .. 1.0) - V ``fake_quant`` calls plus ``torch.cat`` against one
``fake_quant_fork`` into a preallocated tensor - after checking that both give the same bits.

Reported per codec, dtype and direction: the median over the repeats, their min - max spread, and the ratio of
the medians to the first codec's.  Needs a GPU: there is no CPU fallback (a CPU time says nothing here)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_inference_in_distributed_edge_networks_amd import codec as C  # noqa: E402
from llm_inference_in_distributed_edge_networks_amd.codec import wire as W  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters       # us per call


def fork_bench(a, names, x32, out):
    """Per-variant path against the fork; appended to out["results"] as direction "per_variant" / "fork"."""
    B, S, H = a.batch, a.seq, a.hidden
    g = torch.Generator("cuda").manual_seed(1)
    for dtype in (torch.float32, torch.bfloat16):
        x = x32.to(dtype)
        for n in names:
            spec = C.get_codec(n)
            for V in (int(v) for v in a.fork_variants.split(",")):
                imps = [torch.rand(B, S, generator=g, device="cuda") for _ in range(max(1, V // 10))]
                variants = [(v % len(imps), int((1 + v // len(imps) % 10) / 10 * S)) for v in range(V)]
                y = torch.empty(V * B * S, H, dtype=dtype, device="cuda")
                fns = {"per_variant": lambda: torch.cat([C.fake_quant(x, spec, B, S, importance=imps[s], k=k)[0]
                                                         for s, k in variants]),
                       "fork": lambda: C.fake_quant_fork(x, spec, B, S, variants, imps, out=y)[0]}
                bits = torch.int32 if dtype == torch.float32 else torch.int16
                if not torch.equal(fns["per_variant"]().view(bits), fns["fork"]().view(bits)):
                    raise SystemExit(f"{n} {dtype} V={V}: the fork differs from the per-variant path")
                t = {k: [] for k in fns}
                for _ in range(a.repeats):
                    for k, fn in fns.items():
                        t[k].append(timed(fn, a.iters))
                base = statistics.median(t["per_variant"])
                for k in fns:
                    med = statistics.median(t[k])
                    out["results"].append({"dtype": str(dtype).split(".")[-1], "codec": n, "variants": V,
                                           "direction": k, "median_us": round(med, 2), "min_us": round(min(t[k]), 2),
                                           "max_us": round(max(t[k]), 2), "ratio_to_first": round(med / base, 4)})
                    print(f"{str(dtype).split('.')[-1]:8s} {n:18s} V={V:3d} {k:11s} median {med:10.2f} us  "
                          f"[{min(t[k]):.2f}, {max(t[k]):.2f}]  x{med / base:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codecs", default="rgroup,rgroup_rot")
    ap.add_argument("--plan-bits", type=int, default=4, help="uniform group plan of the head-group codecs")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json-out", default="", help="also write the results there as JSON")
    ap.add_argument("--fork-variants", default="", help="e.g. 10,40: time fake_quant_fork against that many "
                                                        "fake_quant calls + torch.cat instead of pack / unpack")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("codec_bench needs a GPU")
    B, S, H = a.batch, a.seq, a.hidden
    names = a.codecs.split(",")
    g = torch.Generator("cuda").manual_seed(0)
    x32 = torch.randn(B * S, H, generator=g, device="cuda") * 2
    x32[:, 70] *= 100
    imp = torch.rand(B, S, generator=g, device="cuda")
    out = {"shape": [B, S, H], "iters": a.iters, "repeats": a.repeats, "plan_bits": a.plan_bits,
           "device": torch.cuda.get_device_name(0), "results": []}
    if a.fork_variants:
        fork_bench(a, names, x32, out)
    for dtype in () if a.fork_variants else (torch.float32, torch.bfloat16):
        x = x32.to(dtype)
        runs = {}
        for n in names:
            base, *mods = n.split("@")
            spec = C.get_codec(base)
            for mod in mods:
                spec = C.with_mx_elem(spec, mod) if mod in W.MX_ELEMS else C.with_mx_rot(spec, "h32") if mod == "rot" \
                    else C.with_outliers(spec, mod) if mod in W.OUTLIERS else C.with_row_rot(spec, mod) \
                    if mod in W.ROW_ROTS else C.with_native_wire(spec, mod)
            if C.wire.needs_plan(spec):
                spec = C.wire.with_plan(spec, (a.plan_bits,) * (H // 64))
            L = C.layout(spec, B, S, H, C.wire.num_lo(spec, a.ratio, S), dtype)
            msg = torch.zeros(L.total, dtype=torch.uint8, device="cuda")
            y = torch.empty(B * S, H, dtype=dtype, device="cuda")
            C.encode(x, spec, B, S, a.ratio, imp, out=msg)          # header, mask, plan and statistics: once
            # the pack kernel alone (the whole encode is several launches and host-bound at this size)
            enc = lambda spec=spec, msg=msg, L=L: W.call(           # noqa: E731
                "edge_pack", W.ptr(x), W.ptr(msg), *W._args(spec, L), int(dtype == torch.float32), W.stream())
            dec = lambda spec=spec, msg=msg, L=L, y=y: C.decode(msg, spec, L, out=y)             # noqa: E731
            for _ in range(10):
                enc()
                dec()
            runs[n] = {"enc": enc, "dec": dec, "bytes": L.total, "pack": [], "unpack": []}
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for n in names:
                runs[n]["pack"].append(timed(runs[n]["enc"], a.iters))
            for n in names:
                runs[n]["unpack"].append(timed(runs[n]["dec"], a.iters))
        for direction in ("pack", "unpack"):
            base = statistics.median(runs[names[0]][direction])
            for n in names:
                t = runs[n][direction]
                med = statistics.median(t)
                row = {"dtype": str(dtype).split(".")[-1], "codec": n, "direction": direction,
                       "message_bytes": runs[n]["bytes"], "median_us": round(med, 2), "min_us": round(min(t), 2),
                       "max_us": round(max(t), 2), "ratio_to_first": round(med / base, 4),
                       "repeats_us": [round(v, 2) for v in t]}
                out["results"].append(row)
                print(f"{row['dtype']:8s} {direction:6s} {n:18s} median {med:8.2f} us  [{min(t):.2f}, {max(t):.2f}]  "
                      f"x{med / base:.3f}  ({runs[n]['bytes']} B)", flush=True)
    if a.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.json_out)), exist_ok=True)
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
