#!/usr/bin/env python3
"""Time the group-scaled fp8 kernels against the per-tile fp8 kernels.

    python tools/fp8_group_probe.py [--out FILE.md] [--group-size 128]

For each geometry the project profiles (64 KiB x 32 layers x 16 blocks,
8 KiB x 80 layers x 16 blocks) it times, through BlockCopier on one GPU:

  gather_fp8        per-tile: amax launch + quantize launch (sum of both)
  gather_fp8_group  per-group: one launch
  scatter_fp8 / scatter_fp8_group

A sample is the device-event time around a burst of back-to-back launches
divided by the burst length; the two variants alternate sample by sample
so drift hits both; the table reports the median and the min..max spread.
GB/s counts the bf16 bytes read (gather) or written (scatter). Needs a
GPU: there is no CPU fallback for a timing.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

GEOMETRIES = [(64 * 1024, 32, 16), (8 * 1024, 80, 16)]


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
        sys.exit("fp8_group_probe needs a GPU")
    from llm_d_kv_cache_amd.ops import block_copier

    gs = args.group_size
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for bb, nl, nb in GEOMETRIES:
        torch.manual_seed(0)
        pages = [(torch.randn(4 * nb, bb // 2, device="cuda") * 3)
                 .to(torch.bfloat16) for _ in range(nl)]
        ids = list(range(1, 1 + 3 * nb, 3))
        copier = block_copier([pages])
        tile_b = copier.packed_bytes_fp8(0, nb)
        scratch_b = copier.fp8_scratch_bytes(0, nb)
        tile_slab = torch.empty(tile_b + scratch_b, dtype=torch.uint8,
                                device="cuda")
        group_slab = torch.empty(copier.packed_bytes_fp8_group(0, nb, gs),
                                 dtype=torch.uint8, device="cuda")
        ops = {
            "gather_fp8": lambda: copier.gather_fp8(
                0, ids, tile_slab.data_ptr(), tile_slab.data_ptr() + tile_b,
                stream),
            "gather_fp8_group": lambda: copier.gather_fp8_group(
                0, ids, group_slab.data_ptr(), gs, stream),
            "scatter_fp8": lambda: copier.scatter_fp8(
                0, ids, tile_slab.data_ptr(), stream),
            "scatter_fp8_group": lambda: copier.scatter_fp8_group(
                0, ids, group_slab.data_ptr(), gs, stream),
        }

        def sample(fn):
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.burst):
                fn()
            end.record()
            end.synchronize()
            return start.elapsed_time(end) * 1e3 / args.burst  # us

        # the gathers fill both slabs before any scatter reads them
        for pair in (("gather_fp8", "gather_fp8_group"),
                     ("scatter_fp8", "scatter_fp8_group")):
            times = {name: [] for name in pair}
            for i in range(args.warmup + args.samples):
                for name in pair:
                    t = sample(ops[name])
                    if i >= args.warmup:
                        times[name].append(t)
            for name in pair:
                ts = sorted(times[name])
                med = statistics.median(ts)
                rows.append({
                    "block_bytes": bb, "layers": nl, "blocks": nb,
                    "kernel": name, "group_size": gs if "group" in name else 0,
                    "median_us": round(med, 2), "min_us": round(ts[0], 2),
                    "max_us": round(ts[-1], 2),
                    "bf16_GBps": round(bb * nl * nb / med / 1e3, 1),
                })
        del copier

    lines = [
        "| geometry | kernel | median us/launch | min..max us | bf16 GB/s |",
        "|---|---|---:|---:|---:|",
    ]
    for r in rows:
        lines.append(
            f"| {r['block_bytes'] // 1024} KiB x {r['layers']} layers x "
            f"{r['blocks']} blocks | {r['kernel']}"
            f"{' (G=%d)' % r['group_size'] if r['group_size'] else ''} | "
            f"{r['median_us']} | {r['min_us']}..{r['max_us']} | "
            f"{r['bf16_GBps']} |")
    table = "\n".join(lines)
    print(table)
    print(json.dumps({"device": torch.cuda.get_device_name(0),
                      "burst": args.burst, "samples": args.samples,
                      "rows": rows}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(table + "\n")


if __name__ == "__main__":
    main()
