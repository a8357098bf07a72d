#!/usr/bin/env python3
"""Launch the fp4 kernels over fp8 pages next to their neighbours, for a
kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/fp8_page_fp4_probe.py
    python tools/fp8_page_fp4_probe.py --summarize DIR [--out FILE.md]

The first form needs a GPU and only launches: at 8 KiB x 80 layers x 16
blocks (10 MiB of pages per launch) it runs, through BlockCopier in one
process and alternating launch by launch,

  gather / scatter                    raw copies (kvc_gather_blocks,
                                      kvc_scatter_blocks)
  gather_fp4_group, bf16 pages        kvc_gather_fp4_group, G=32 and 128
  gather_fp4_group, fp8 pages         kvc_gather_fp4_group_fp8page, G=32, 128
  scatter_fp4_group, fp8 pages        kvc_scatter_fp4_group_fp8page, G=32, 128

so every kernel reads (gather) or writes (scatter) the same number of page
bytes. The timing comes from the profiler's per-dispatch records, not from
this script. The second form needs no GPU: it reads the *kernel_trace.csv
the profiler wrote under DIR and prints median, min and max per kernel and
the page bytes moved per second at the median.
"""
import argparse
import csv
import re
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

BLOCK_BYTES, LAYERS, BLOCKS = 8 * 1024, 80, 16
GROUP_SIZES = (32, 128)
PAGE_BYTES = BLOCK_BYTES * LAYERS * BLOCKS


def launch(rounds, warmup):
    import torch

    if not torch.cuda.is_available():
        sys.exit("fp8_page_fp4_probe needs a GPU to launch")
    from llm_d_kv_cache_amd.ops import block_copier

    torch.manual_seed(0)
    nblk = 4 * BLOCKS
    bf16 = [(torch.randn(nblk, BLOCK_BYTES // 2, device="cuda") * 3)
            .to(torch.bfloat16) for _ in range(LAYERS)]
    fp8 = [(torch.randn(nblk, BLOCK_BYTES) * 3).to(torch.float8_e4m3fn).cuda()
           for _ in range(LAYERS)]
    ids = list(range(1, 1 + 3 * BLOCKS, 3))
    c16 = block_copier([bf16])
    c8 = block_copier([fp8])
    stream = torch.cuda.current_stream().cuda_stream

    def slab(nbytes):
        return torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    raw = slab(c8.packed_bytes(0, BLOCKS))
    s16 = {g: slab(c16.packed_bytes_fp4_group(0, BLOCKS, g))
           for g in GROUP_SIZES}
    s8 = {g: slab(c8.packed_bytes_fp4_group(0, BLOCKS, g))
          for g in GROUP_SIZES}
    # every gather comes before the scatter that reads its slab
    ops = [lambda: c8.gather(0, ids, raw.data_ptr(), stream),
           lambda: c8.scatter(0, ids, raw.data_ptr(), stream)]
    for g in GROUP_SIZES:
        ops += [
            lambda g=g: c16.gather_fp4_group(0, ids, s16[g].data_ptr(), g,
                                             stream),
            lambda g=g: c8.gather_fp4_group(0, ids, s8[g].data_ptr(), g,
                                            stream),
            lambda g=g: c8.scatter_fp4_group(0, ids, s8[g].data_ptr(), g,
                                             stream),
        ]
    for i in range(warmup + rounds):
        for op in ops:
            op()
        if i % 16 == 15:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    print(f"launched {len(ops)} kernels x {warmup + rounds} rounds on "
          f"{torch.cuda.get_device_name(0)}")


# kernel name in the trace -> row label; template arguments pick G
def _label(name):
    m = re.search(r"kvc_(gather|scatter)_blocks", name)
    if m:
        return f"kvc_{m.group(1)}_blocks (raw)"
    m = re.search(r"kvc_gather_fp4_group_fp8page<(\d+)", name)
    if m:
        return f"kvc_gather_fp4_group_fp8page (G={16 * int(m.group(1))})"
    if "kvc_scatter_fp4_group_fp8page" in name:
        return "kvc_scatter_fp4_group_fp8page (G={})"
    m = re.search(r"kvc_gather_fp4_group<(\d+)", name)
    if m:
        return f"kvc_gather_fp4_group, bf16 pages (G={8 * int(m.group(1))})"
    return None


def summarize(directory, warmup, out):
    files = sorted(Path(directory).rglob("*kernel_trace.csv"))
    if not files:
        sys.exit(f"no *kernel_trace.csv under {directory}")
    times = {}
    scatters = 0
    for f in files:
        with open(f, newline="") as fh:
            rows = sorted(csv.DictReader(fh),
                          key=lambda r: int(r["Start_Timestamp"]))
            for row in rows:
                label = _label(row["Kernel_Name"])
                if label is None:
                    continue
                if "{}" in label:
                    # one kernel for every G (the lane shift is an argument):
                    # launch() alternates the group sizes, in order
                    scatters += 1
                    label = label.format(
                        GROUP_SIZES[(scatters - 1) % len(GROUP_SIZES)])
                dt = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
                times.setdefault(label, []).append(dt / 1e3)  # us
    lines = ["| kernel | dispatches | median us | min..max us | page GB/s |",
             "|---|---:|---:|---:|---:|"]
    for label in sorted(times):
        # the first `warmup` dispatches of every kernel are dropped
        ts = sorted(times[label][warmup:])
        med = statistics.median(ts)
        lines.append(f"| {label} | {len(ts)} | {med:.2f} | "
                     f"{ts[0]:.2f}..{ts[-1]:.2f} | "
                     f"{PAGE_BYTES / med / 1e3:.0f} |")
    table = "\n".join(lines)
    print(table)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(table + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--summarize", type=str, default="")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize, args.warmup, args.out)
    else:
        launch(args.rounds, args.warmup)


if __name__ == "__main__":
    main()
