#!/usr/bin/env python3
"""Time the group-scaled fp4 kernels against the group-scaled fp8 kernels.

    python tools/fp4_group_probe.py [--out FILE.md]

For each geometry the project profiles (64 KiB x 32 layers x 16 blocks,
8 KiB x 80 layers x 16 blocks) it times, through BlockCopier on one GPU and
in one run:

  gather_fp8_group  (G=128)       scatter_fp8_group  (G=128)
  gather_fp4_group  (G=32, G=128) scatter_fp4_group  (G=32, G=128)

Same sampling as tools/fp8_group_probe.py: a sample is the device-event
time around a burst of back-to-back launches divided by the burst length;
the variants alternate sample by sample so drift hits all of them; the
table reports the median and the min..max spread. GB/s counts the bf16
bytes read (gather) or written (scatter). The last column compares each
fp4 median with the fp8-group median plus the band (max - min) the
fp8-group samples of the same run show. Needs a GPU: there is no CPU
fallback for a timing.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

GEOMETRIES = [(64 * 1024, 32, 16), (8 * 1024, 80, 16)]
FP8_G = 128
FP4_GS = (32, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--samples", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("fp4_group_probe needs a GPU")
    from llm_d_kv_cache_amd.ops import block_copier

    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for bb, nl, nb in GEOMETRIES:
        torch.manual_seed(0)
        pages = [(torch.randn(4 * nb, bb // 2, device="cuda") * 3)
                 .to(torch.bfloat16) for _ in range(nl)]
        ids = list(range(1, 1 + 3 * nb, 3))
        copier = block_copier([pages])
        fp8_slab = torch.empty(copier.packed_bytes_fp8_group(0, nb, FP8_G),
                               dtype=torch.uint8, device="cuda")
        fp4_slabs = {
            g: torch.empty(copier.packed_bytes_fp4_group(0, nb, g),
                           dtype=torch.uint8, device="cuda")
            for g in FP4_GS}

        def fp4_op(kind, g):
            fn = getattr(copier, f"{kind}_fp4_group")
            return lambda: fn(0, ids, fp4_slabs[g].data_ptr(), g, stream)

        ops = {
            "gather": [("gather_fp8_group", FP8_G,
                        lambda: copier.gather_fp8_group(
                            0, ids, fp8_slab.data_ptr(), FP8_G, stream))] +
                      [("gather_fp4_group", g, fp4_op("gather", g))
                       for g in FP4_GS],
            "scatter": [("scatter_fp8_group", FP8_G,
                         lambda: copier.scatter_fp8_group(
                             0, ids, fp8_slab.data_ptr(), FP8_G, stream))] +
                       [("scatter_fp4_group", g, fp4_op("scatter", g))
                        for g in FP4_GS],
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

        # the gathers fill every slab before any scatter reads them
        for kind in ("gather", "scatter"):
            times = {(name, g): [] for name, g, _ in ops[kind]}
            for i in range(args.warmup + args.samples):
                for name, g, fn in ops[kind]:
                    t = sample(fn)
                    if i >= args.warmup:
                        times[(name, g)].append(t)
            ref = sorted(times[(f"{kind}_fp8_group", FP8_G)])
            limit = statistics.median(ref) + (ref[-1] - ref[0])
            for name, g, _ in ops[kind]:
                ts = sorted(times[(name, g)])
                med = statistics.median(ts)
                rows.append({
                    "block_bytes": bb, "layers": nl, "blocks": nb,
                    "kernel": name, "group_size": g,
                    "median_us": round(med, 2), "min_us": round(ts[0], 2),
                    "max_us": round(ts[-1], 2),
                    "bf16_GBps": round(bb * nl * nb / med / 1e3, 1),
                    "limit_us": round(limit, 2),
                    "verdict": ("reference" if "fp8" in name else
                                "within" if med <= limit else "MISSES"),
                })
        del copier

    lines = [
        "| geometry | kernel | median us/launch | min..max us | bf16 GB/s "
        "| vs fp8-group median + band |",
        "|---|---|---:|---:|---:|---|",
    ]
    for r in rows:
        verdict = r["verdict"] if r["verdict"] == "reference" else \
            f"{r['verdict']} ({r['median_us']} vs {r['limit_us']})"
        lines.append(
            f"| {r['block_bytes'] // 1024} KiB x {r['layers']} layers x "
            f"{r['blocks']} blocks | {r['kernel']} (G={r['group_size']}) | "
            f"{r['median_us']} | {r['min_us']}..{r['max_us']} | "
            f"{r['bf16_GBps']} | {verdict} |")
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
