#!/usr/bin/env python3
"""Measure what per-record checksums cost.

    python tools/checksum_probe.py [--out FILE.md]

Part 1, kernels. For each geometry the project profiles (64 KiB x 32 layers
x 16 blocks, 8 KiB x 80 layers x 16 blocks) it times, through BlockCopier on
one GPU and over the same bytes:

  gather   raw kvc_gather_blocks into a slab with footers (the yardstick)
  seal     kvc_record_partial_sums + kvc_seal_records (two launches)
  verify   kvc_record_partial_sums + kvc_verify_records, the stream sync
           and the read of the two result words (verify_records returns a
           verdict, so every call ends in a sync: this is a call time, not
           a kernel time)

gather and seal samples are the device-event time around a burst of
back-to-back launches divided by the burst length; a verify sample is the
host clock around the same number of calls. The variants alternate sample
by sample so drift hits all of them; the table reports the median and the
min..max spread. GB/s counts the payload bytes read once.

Part 2, end to end. Engine store and load in raw mode on the staged path,
checksum on against off (off is the engine as it was before the option
existed), same process, alternating sample by sample: one sample stores
--files files of 64 KiB x 32 layers x 16 blocks and loads them back. The
load figure includes the per-file sync the verdict needs.

Needs a GPU: there is no CPU fallback for a timing.
"""
import argparse
import json
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

GEOMETRIES = [(64 * 1024, 32, 16), (8 * 1024, 80, 16)]


def _stats(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[0], ts[-1]


def kernel_rows(args, torch):
    from llm_d_kv_cache_amd.ops import block_copier

    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for bb, nl, nb in GEOMETRIES:
        torch.manual_seed(0)
        pages = [torch.randint(0, 255, (4 * nb, bb), dtype=torch.uint8,
                               device="cuda") for _ in range(nl)]
        ids = list(range(1, 1 + 3 * nb, 3))
        copier = block_copier([pages])
        tiles = nb * nl
        slab = torch.empty(copier.packed_bytes(0, nb, checksum=True),
                           dtype=torch.uint8, device="cuda")

        def gather():
            copier.gather(0, ids, slab.data_ptr(), stream, checksum=True)

        def seal():
            copier.seal_records(slab.data_ptr(), tiles, bb, stream)

        def verify():
            bad, first = copier.verify_records(slab.data_ptr(), tiles, bb,
                                               stream)
            assert (bad, first) == (0, -1), (bad, first)

        def device_sample(fn):
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.burst):
                fn()
            end.record()
            end.synchronize()
            return start.elapsed_time(end) * 1e3 / args.burst  # us

        def host_sample(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.burst):
                fn()
            return (time.perf_counter() - t0) * 1e6 / args.burst  # us

        ops = [("gather", gather, device_sample),
               ("seal", seal, device_sample),
               ("verify+sync", verify, host_sample)]
        gather()
        seal()
        times = {name: [] for name, _, _ in ops}
        for i in range(args.warmup + args.samples):
            for name, fn, sampler in ops:
                t = sampler(fn)
                if i >= args.warmup:
                    times[name].append(t)
        for name, _, _ in ops:
            med, lo, hi = _stats(times[name])
            rows.append({
                "block_bytes": bb, "layers": nl, "blocks": nb, "op": name,
                "median_us": round(med, 2), "min_us": round(lo, 2),
                "max_us": round(hi, 2),
                "payload_GBps": round(bb * nl * nb / med / 1e3, 1),
            })
        del copier
    return rows


def engine_rows(args, torch):
    from llm_d_kv_cache_amd.offload import (
        FileMapper, GPUToStorageHandler, KVCacheLayoutConfig,
        OffloadEngineConfig, StorageToGPUHandler, TorchOffloadEngine)

    bb, nl, bpf = GEOMETRIES[0]
    n_blocks = bpf * args.files
    pages = [torch.randint(0, 255, (n_blocks, bb), dtype=torch.uint8,
                           device="cuda") for _ in range(nl)]
    ids = list(range(n_blocks))
    payload = n_blocks * nl * bb
    root = Path(tempfile.mkdtemp(prefix="kvc_ckprobe_", dir=args.dir or None))
    variants = {}
    for ck in (False, True):
        eng = TorchOffloadEngine(
            [pages], OffloadEngineConfig(io_threads=args.io_threads,
                                         gpu_blocks_per_file=bpf,
                                         checksum=ck))
        mapper = FileMapper(str(root), KVCacheLayoutConfig(
            model="ckprobe", dtype="uint8+ck" if ck else "uint8"))
        variants[ck] = (eng, GPUToStorageHandler(eng, mapper, [bpf]),
                        StorageToGPUHandler(eng, mapper, [bpf]))

    def wait(handler):
        deadline = time.time() + 120
        while time.time() < deadline:
            fin = handler.get_finished()
            if fin:
                assert fin[0].success, "transfer failed"
                return
            time.sleep(0.0005)
        raise SystemExit("transfer timed out")

    times = {(ck, op): [] for ck in variants for op in ("store", "load")}
    try:
        for i in range(args.warmup + args.e2e_samples):
            for ck, (eng, store, load) in variants.items():
                hashes = [0x1000 * (i + 1) + f for f in range(args.files)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                store.transfer_async(hashes, {0: ids})
                wait(store)
                t1 = time.perf_counter()
                load.transfer_async(hashes, {0: ids})
                wait(load)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if i >= args.warmup:
                    times[(ck, "store")].append(payload / (t1 - t0) / 1e9)
                    times[(ck, "load")].append(payload / (t2 - t1) / 1e9)
                for sub in root.iterdir():
                    shutil.rmtree(sub, ignore_errors=True)
        for ck, (eng, _, _) in variants.items():
            st = eng.stats()
            assert st.checksum_failures == 0 and st.errors == 0
    finally:
        variants.clear()
        shutil.rmtree(root, ignore_errors=True)
    rows = []
    for op in ("store", "load"):
        off = _stats(times[(False, op)])
        on = _stats(times[(True, op)])
        rows.append({
            "op": op, "files": args.files, "payload_MiB": payload >> 20,
            "off_GBps": round(off[0], 2),
            "off_range": [round(off[1], 2), round(off[2], 2)],
            "on_GBps": round(on[0], 2),
            "on_range": [round(on[1], 2), round(on[2], 2)],
            "on_over_off": round(on[0] / off[0], 3),
        })
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--samples", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--e2e-samples", type=int, default=9)
    ap.add_argument("--io-threads", type=int, default=8)
    ap.add_argument("--dir", type=str, default="",
                    help="directory for the end-to-end files")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("checksum_probe needs a GPU")

    krows = kernel_rows(args, torch)
    lines = [
        "| geometry | op | median us | min..max us | payload GB/s |",
        "|---|---|---:|---:|---:|",
    ]
    for r in krows:
        lines.append(
            f"| {r['block_bytes'] // 1024} KiB x {r['layers']} layers x "
            f"{r['blocks']} blocks | {r['op']} | {r['median_us']} | "
            f"{r['min_us']}..{r['max_us']} | {r['payload_GBps']} |")
    erows = [] if args.skip_e2e else engine_rows(args, torch)
    if erows:
        lines += [
            "",
            "| engine op | payload MiB | off GB/s (min..max) | "
            "on GB/s (min..max) | on / off |",
            "|---|---:|---:|---:|---:|",
        ]
        for r in erows:
            lines.append(
                f"| {r['op']} | {r['payload_MiB']} | {r['off_GBps']} "
                f"({r['off_range'][0]}..{r['off_range'][1]}) | "
                f"{r['on_GBps']} ({r['on_range'][0]}..{r['on_range'][1]}) | "
                f"{r['on_over_off']} |")
    table = "\n".join(lines)
    print(table)
    print(json.dumps({"device": torch.cuda.get_device_name(0),
                      "burst": args.burst, "samples": args.samples,
                      "kernels": krows, "engine": erows}))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(table + "\n")


if __name__ == "__main__":
    main()
