#!/usr/bin/env python3
"""Time the fp8 MLA kernels against the flat kernels on the same pages.

    python tools/fp8_ds_mla_probe.py [--out FILE.md]

Geometry of the DeepSeek MLA preset: 16-token blocks of 576-wide rows
(18 KiB tiles), 61 layers, 16 blocks per launch. Through BlockCopier on one
GPU it times

  gather_fp8_mla / scatter_fp8_mla     one wave per token row
  gather_fp8_group / scatter_fp8_group at G = 64 (kvc_gather_fp8_group<8>),
                                       the flat kernels on identical input
  gather                               the raw copy (kvc_gather_blocks)

A sample is the device-event time around a burst of back-to-back launches
divided by the burst length; the kernels of a pair alternate sample by
sample so drift hits all of them; the table reports the median and the
min..max spread, the bytes a launch reads plus writes, and the resulting
TB/s. Needs a GPU: there is no CPU fallback for a timing.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ROWS, LAYERS, BLOCKS = 16, 61, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--samples", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("fp8_ds_mla_probe needs a GPU")
    from llm_d_kv_cache_amd.ops import block_copier

    bb = ROWS * 1152
    torch.manual_seed(0)
    pages = [(torch.randn(4 * BLOCKS, bb // 2, device="cuda") * 3)
             .to(torch.bfloat16) for _ in range(LAYERS)]
    ids = list(range(1, 1 + 3 * BLOCKS, 3))
    copier = block_copier([pages])
    stream = torch.cuda.current_stream().cuda_stream
    raw_b = copier.packed_bytes(0, BLOCKS)
    mla_b = copier.packed_bytes_fp8_mla(0, BLOCKS)
    grp_b = copier.packed_bytes_fp8_group(0, BLOCKS, 64)
    slabs = {n: torch.empty(b, dtype=torch.uint8, device="cuda")
             for n, b in (("raw", raw_b), ("mla", mla_b), ("grp", grp_b))}
    ptr = {n: t.data_ptr() for n, t in slabs.items()}
    # name -> (call, bytes read + written per launch)
    ops = {
        "gather_fp8_mla": (lambda: copier.gather_fp8_mla(
            0, ids, ptr["mla"], stream), raw_b + mla_b),
        "gather_fp8_group (G=64)": (lambda: copier.gather_fp8_group(
            0, ids, ptr["grp"], 64, stream), raw_b + grp_b),
        "gather (raw)": (lambda: copier.gather(
            0, ids, ptr["raw"], stream), 2 * raw_b),
        "scatter_fp8_mla": (lambda: copier.scatter_fp8_mla(
            0, ids, ptr["mla"], stream), raw_b + mla_b),
        "scatter_fp8_group (G=64)": (lambda: copier.scatter_fp8_group(
            0, ids, ptr["grp"], 64, stream), raw_b + grp_b),
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

    rows = []
    # the gathers fill the slabs before any scatter reads them
    for group in (list(ops)[:3], list(ops)[3:]):
        times = {name: [] for name in group}
        for i in range(args.warmup + args.samples):
            for name in group:
                t = sample(ops[name][0])
                if i >= args.warmup:
                    times[name].append(t)
        for name in group:
            ts = sorted(times[name])
            med = statistics.median(ts)
            rows.append({"kernel": name, "median_us": round(med, 2),
                         "min_us": round(ts[0], 2), "max_us": round(ts[-1], 2),
                         "bytes": ops[name][1],
                         "TBps": round(ops[name][1] / med / 1e6, 2)})

    lines = ["| kernel | median us/launch | min..max us | bytes read + "
             "written | TB/s |", "|---|---:|---:|---:|---:|"]
    for r in rows:
        lines.append(f"| {r['kernel']} | {r['median_us']} | {r['min_us']}.."
                     f"{r['max_us']} | {r['bytes']} | {r['TBps']} |")
    table = "\n".join(lines)
    print(table)
    print(json.dumps({"device": torch.cuda.get_device_name(0),
                      "rows_per_tile": ROWS, "layers": LAYERS,
                      "blocks": BLOCKS, "burst": args.burst,
                      "samples": args.samples, "rows": rows}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(table + "\n")


if __name__ == "__main__":
    main()
