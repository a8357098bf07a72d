#!/usr/bin/env python3
"""Time the fp16 instantiations of the fp8 kernels against their bf16 twins.

    python tools/fp8_fp16_probe.py [--out FILE.md] [--group-size 128]

At the 64 KiB x 32 layers x 16 blocks geometry it times, through two
BlockCopiers over the same page bytes (one built with kv_dtype="bfloat16",
one with "float16"), on one GPU:

  gather_fp8        per-tile: amax launch + quantize launch (sum of both)
  gather_fp8_group  per-group: one launch
  scatter_fp8 / scatter_fp8_group

A sample is the device-event time around a burst of back-to-back launches
divided by the burst length; the bf16 and fp16 twins alternate sample by
sample so drift hits both; the table reports the median and the min..max
spread. The same bytes move either way, so parity is the expectation. Run
it under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for
per-dispatch times. Needs a GPU: there is no CPU fallback for a timing.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

GEOMETRY = (64 * 1024, 32, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--samples", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("fp8_fp16_probe needs a GPU")
    from llm_d_kv_cache_amd.ops import block_copier

    gs = args.group_size
    bb, nl, nb = GEOMETRY
    stream = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    # values finite and normal in both formats, one buffer per format so
    # each kernel reads numbers, not the other format's bit patterns
    vals = [torch.randn(4 * nb, bb // 2, device="cuda") * 3 for _ in range(nl)]
    ids = list(range(1, 1 + 3 * nb, 3))
    ops = {}
    keep = []
    for name, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        pages = [v.to(dtype) for v in vals]
        copier = block_copier([pages])
        tile_b = copier.packed_bytes_fp8(0, nb)
        tile_slab = torch.empty(tile_b + copier.fp8_scratch_bytes(0, nb),
                                dtype=torch.uint8, device="cuda")
        group_slab = torch.empty(copier.packed_bytes_fp8_group(0, nb, gs),
                                 dtype=torch.uint8, device="cuda")
        keep.append((pages, copier, tile_slab, group_slab))
        ops[name] = {
            "gather_fp8": lambda c=copier, s=tile_slab, b=tile_b:
                c.gather_fp8(0, ids, s.data_ptr(), s.data_ptr() + b, stream),
            "gather_fp8_group": lambda c=copier, s=group_slab:
                c.gather_fp8_group(0, ids, s.data_ptr(), gs, stream),
            "scatter_fp8": lambda c=copier, s=tile_slab:
                c.scatter_fp8(0, ids, s.data_ptr(), stream),
            "scatter_fp8_group": lambda c=copier, s=group_slab:
                c.scatter_fp8_group(0, ids, s.data_ptr(), gs, stream),
        }
    del vals

    def sample(fn):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.burst):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / args.burst  # us

    rows = []
    # the gathers fill the slabs before any scatter reads them
    for kernel in ("gather_fp8", "gather_fp8_group", "scatter_fp8",
                   "scatter_fp8_group"):
        times = {"bf16": [], "fp16": []}
        for i in range(args.warmup + args.samples):
            for fmt in ("bf16", "fp16"):
                t = sample(ops[fmt][kernel])
                if i >= args.warmup:
                    times[fmt].append(t)
        med = {}
        for fmt in ("bf16", "fp16"):
            ts = sorted(times[fmt])
            med[fmt] = statistics.median(ts)
            rows.append({
                "kernel": kernel, "pages": fmt,
                "group_size": gs if "group" in kernel else 0,
                "median_us": round(med[fmt], 2), "min_us": round(ts[0], 2),
                "max_us": round(ts[-1], 2),
                "page_GBps": round(bb * nl * nb / med[fmt] / 1e3, 1),
            })
        rows[-1]["fp16_over_bf16"] = round(med["fp16"] / med["bf16"], 3)

    lines = [
        "| kernel | pages | median us/launch | min..max us | page GB/s | "
        "fp16/bf16 |",
        "|---|---|---:|---:|---:|---:|",
    ]
    for r in rows:
        lines.append(
            f"| {r['kernel']}"
            f"{' (G=%d)' % r['group_size'] if r['group_size'] else ''} | "
            f"{r['pages']} | {r['median_us']} | "
            f"{r['min_us']}..{r['max_us']} | {r['page_GBps']} | "
            f"{r.get('fp16_over_bf16', '')} |")
    table = "\n".join(lines)
    print(table)
    print(json.dumps({"device": torch.cuda.get_device_name(0),
                      "geometry": GEOMETRY, "burst": args.burst,
                      "samples": args.samples, "rows": rows}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(table + "\n")


if __name__ == "__main__":
    main()
