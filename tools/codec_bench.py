"""Pack / unpack time of boundary codecs against each other in one process (device events, alternating repeats).

    python tools/codec_bench.py --codecs rgroup,rgroup_rot --plan-bits 4 --json-out OUT/codec_bench.json
    python tools/codec_bench.py --codecs passthrough,passthrough@bf16,passthrough@fp16,passthrough@fp16s

``name@wire`` is codec ``name`` with its activation-dtype rows on the 16-bit wire ``wire`` (``with_native_wire``).

Every codec packs the same activations ([B * S, H], randn with one massive channel) into its own preallocated
message (the pack kernel alone: selection and statistics run once, before) and decodes it into a preallocated
tensor; a repeat times ``--iters`` back-to-back calls of one direction
between two events, and the codecs alternate within every repeat so that clock and neighbour drift hit all alike.
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
    for dtype in (torch.float32, torch.bfloat16):
        x = x32.to(dtype)
        runs = {}
        for n in names:
            spec = C.with_native_wire(C.get_codec(n.split("@")[0]), (n.split("@") + ["native"])[1])
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
