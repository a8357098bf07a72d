"""Torch-facing construction of the native offload engine.

Tensors are handed to C++ as raw (pointer, stride, bytes) descriptors; the
native module has no libtorch dependency. On a GPU box the engine REQUIRES
the HIP extension and CUDA(=HIP) tensors — there is no silent eager
fallback; ``copy_path='host'`` on CPU tensors is an explicit mode used by
CPU-only CI.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence

DEFAULT_STAGING_BUDGET_BYTES = 150 * 1024**3  # parity with reference worker.py:70


@dataclass
class OffloadEngineConfig:
    io_threads: int = 16
    gpu_blocks_per_file: int = 16
    read_preferring_ratio: float = 0.75
    max_write_queued_seconds: float = 30.0
    copy_path: str = "staged"  # staged | zero_copy | host
    # raw | fp8_e4m3 (16-bit float pages -> fp8 + one scale per (block,
    # layer) tile)
    # | fp8_e4m3_group (fp8 + one scale per fp8_group_size elements)
    # | fp4_e2m1_group (4-bit e2m1 codes, two per byte, + one scale per
    #   fp4_group_size elements; lossy at 4 bits, model quality unmeasured)
    serialize: str = "raw"
    # elements per scale for fp8_e4m3_group (set it to head_dim); one of
    # 64/128/256/512, ignored by the other modes
    fp8_group_size: int = 128
    # elements per scale for fp4_e2m1_group; one of 16/32/64/128, ignored by
    # the other modes
    fp4_group_size: int = 32
    host_cache_bytes: int = 0  # pinned-DRAM cache tier (0 = off)
    write_policy: str = "through"  # through | back (flush async via DRAM tier)
    direct_io: bool = False    # O_DIRECT for NVMe (auto-fallback elsewhere)
    # per-record checksums: every (block, layer) record gains a 16-byte
    # footer, sealed on store and verified on load before any KV page is
    # written. Give the FileMapper a dtype tag ending in "+ck" so files with
    # and without footers never share a directory.
    checksum: bool = False
    device: int = 0
    staging_budget_bytes: int = DEFAULT_STAGING_BUDGET_BYTES
    # page format the fp8 and fp4 modes convert from/to: auto | bfloat16 |
    # float16 | float8_e4m3fn.
    # auto = float16 if every KV tensor is torch.float16, float8_e4m3fn if
    # every one is torch.float8_e4m3fn, else bfloat16; an explicit value
    # covers opaque uint8 views. float8_e4m3fn pages (an fp8 KV cache) are a
    # source of fp4_e2m1_group only; the fp8 modes raise on them. Ignored by
    # serialize="raw".
    kv_dtype: str = "auto"


SERIALIZE_MODES = ("raw", "fp8_e4m3", "fp8_e4m3_group", "fp4_e2m1_group")
FP8_GROUP_SIZES = (64, 128, 256, 512)
FP4_GROUP_SIZES = (16, 32, 64, 128)
CHECKSUM_FOOTER_BYTES = 16
CHECKSUM_MAGIC = 0x5343564B  # the bytes "KVCS"
# suffix of the FileMapper dtype tag that keeps checksummed files apart
CHECKSUM_DTYPE_SUFFIX = "+ck"
KV_DTYPES = ("bfloat16", "float16", "float8_e4m3fn")
# bytes per page element
KV_DTYPE_BYTES = {"bfloat16": 2, "float16": 2, "float8_e4m3fn": 1}


def resolve_kv_dtype(groups: Sequence[Sequence], kv_dtype: str = "auto",
                     fp8: bool = True) -> str:
    """Page format the fp8 and fp4 codecs convert with: "bfloat16",
    "float16" or "float8_e4m3fn".

    ``auto`` is float16 if every KV tensor is ``torch.float16``,
    float8_e4m3fn if every one is ``torch.float8_e4m3fn``, and bfloat16
    otherwise (bf16 tensors, and the opaque uint8 views of bf16 bits that
    predate this option). An explicit value covers uint8 views of fp16 or
    fp8 pages. Raises ValueError for a value outside
    auto|bfloat16|float16|float8_e4m3fn, and, when ``fp8`` is true, for an
    engine that mixes float16, bfloat16 and float8_e4m3fn tensors, an
    explicit value that contradicts a tensor's own float dtype (either
    direction), or a ``torch.float8_e4m3fnuz`` / ``torch.float8_e5m2``
    tensor (no codec reads those pages). ``fp8=False`` (serialize="raw")
    never converts, so nothing is checked beyond the spelling; every other
    mode, fp4_e2m1_group included, is a converting mode and passes
    ``fp8=True``."""
    import torch

    if kv_dtype not in ("auto",) + KV_DTYPES:
        raise ValueError(
            f"kv_dtype must be one of auto|{'|'.join(KV_DTYPES)}, "
            f"got {kv_dtype!r}")
    names = {torch.float16: "float16", torch.bfloat16: "bfloat16",
             torch.float8_e4m3fn: "float8_e4m3fn"}
    unsupported = (torch.float8_e4m3fnuz, torch.float8_e5m2)
    tensors = [t for g in groups for t in g]
    seen = {names[t.dtype] for t in tensors if t.dtype in names}
    if fp8:
        for t in tensors:
            if t.dtype in unsupported:
                raise ValueError(
                    f"KV tensors of dtype {t.dtype} cannot be converted: the "
                    "only fp8 page format is float8_e4m3fn (OCP); use "
                    "serialize='raw'")
        if len(seen) > 1:
            raise ValueError(
                f"KV tensors mix {' and '.join(sorted(seen))}; the fp8 and "
                "fp4 codecs need one page format per engine")
        if kv_dtype != "auto" and seen and kv_dtype not in seen:
            raise ValueError(
                f"kv_dtype={kv_dtype!r} contradicts KV tensors of dtype "
                f"torch.{next(iter(seen))}")
    if kv_dtype != "auto":
        return kv_dtype
    for dtype in (torch.float16, torch.float8_e4m3fn):
        if tensors and all(t.dtype == dtype for t in tensors):
            return names[dtype]
    return "bfloat16"


def check_serialize_kv_dtype(serialize: str, kv_dtype: str) -> None:
    """float8_e4m3fn pages already are fp8: the fp8 modes raise ValueError on
    them. ``kv_dtype`` is a resolved value (resolve_kv_dtype)."""
    if kv_dtype == "float8_e4m3fn" and serialize in ("fp8_e4m3",
                                                     "fp8_e4m3_group"):
        raise ValueError(
            f"serialize={serialize!r} does not apply to kv_dtype="
            "'float8_e4m3fn' pages, they already are fp8; use 'raw' or "
            "'fp4_e2m1_group'")


def tile_record_bytes(serialize: str, block_bytes: int, fp8_group_size: int,
                      group: int = 0, checksum: bool = False,
                      fp4_group_size: int = 32, *,
                      kv_dtype: str = "bfloat16") -> int:
    """Bytes one (block, layer) tile occupies in a file/object/slab.

    raw: block_bytes. fp8_e4m3: n + 4 (n = block_bytes/2 fp8 bytes, one f32
    scale). fp8_e4m3_group: n + 4*n/G (one f32 scale per G elements).
    fp4_e2m1_group: n/2 + 4*n/G with G = fp4_group_size (two e2m1 codes per
    byte). kv_dtype is the resolved page format: with "float8_e4m3fn" a tile
    holds n = block_bytes elements, so fp4_e2m1_group gives block_bytes/2 +
    4*block_bytes/G; the fp8 modes raise on such pages. checksum=True adds
    the 16-byte footer (sum u64, magic, payload bytes). Raises ValueError
    for an unknown mode or page format, a group size outside FP8_GROUP_SIZES
    (FP4_GROUP_SIZES for fp4), or a KV group whose tile G does not divide.
    """
    if kv_dtype not in KV_DTYPES:
        raise ValueError(
            f"kv_dtype must be one of {'|'.join(KV_DTYPES)}, got {kv_dtype!r}")
    check_serialize_kv_dtype(serialize, kv_dtype)
    footer = CHECKSUM_FOOTER_BYTES if checksum else 0
    if serialize == "raw":
        return block_bytes + footer
    if serialize == "fp8_e4m3":
        return block_bytes // 2 + 4 + footer
    if serialize == "fp4_e2m1_group":
        if fp4_group_size not in FP4_GROUP_SIZES:
            raise ValueError(
                f"fp4_group_size must be one of {FP4_GROUP_SIZES}, "
                f"got {fp4_group_size}")
        width = KV_DTYPE_BYTES[kv_dtype]
        n = block_bytes // width
        if block_bytes % 16 != 0 or n % fp4_group_size != 0:
            raise ValueError(
                f"KV group {group}: block_bytes={block_bytes} holds {n} "
                f"{8 * width}-bit elements, not a multiple of "
                f"fp4_group_size={fp4_group_size}")
        return n // 2 + 4 * (n // fp4_group_size) + footer
    if serialize != "fp8_e4m3_group":
        raise ValueError(
            f"serialize must be one of {'|'.join(SERIALIZE_MODES)}, "
            f"got {serialize!r}")
    if fp8_group_size not in FP8_GROUP_SIZES:
        raise ValueError(
            f"fp8_group_size must be one of {FP8_GROUP_SIZES}, "
            f"got {fp8_group_size}")
    n = block_bytes // 2
    if block_bytes % 16 != 0 or n % fp8_group_size != 0:
        raise ValueError(
            f"KV group {group}: block_bytes={block_bytes} holds {n} bf16 "
            f"elements, not a multiple of fp8_group_size={fp8_group_size}")
    return n + 4 * (n // fp8_group_size) + footer


def record_checksum(buffer) -> int:
    """The ``sum`` field of a record's checksum footer, computed on the host
    over ``buffer`` (bytes-like or a C-contiguous array; length a multiple
    of 4): sum of splitmix64-finalized ``((i + 1) << 32) | word[i]`` mod
    2**64. Same value the seal/verify kernels compute."""
    from .. import ensure_offload_native

    return int(ensure_offload_native().record_checksum(buffer))


class TorchOffloadEngine:
    """Owns the native StorageOffloadEngine built from torch KV tensors.

    groups: one entry per KV-cache group; each a list of per-layer tensors
    shaped (num_blocks, ...) with block-contiguous rows.
    """

    def __init__(self, groups: Sequence[Sequence], config: OffloadEngineConfig):
        import torch

        from .. import ensure_offload_native

        self._ko = ensure_offload_native()
        self.config = config

        if not groups or not groups[0]:
            raise ValueError("need at least one group with one layer tensor")
        first = groups[0][0]
        gpu_mode = first.is_cuda
        for g in groups:
            for t in g:
                if t.is_cuda != gpu_mode:
                    raise ValueError("all KV tensors must live on the same device kind")
        if gpu_mode and config.copy_path == "host":
            raise ValueError("copy_path='host' is invalid for GPU tensors")
        if not gpu_mode and config.copy_path != "host":
            # Explicit: CPU tensors run the host path. Constructing with GPU
            # copy paths on CPU tensors is a config error, not a fallback.
            raise ValueError(
                f"copy_path='{config.copy_path}' requires GPU tensors; "
                "use copy_path='host' for CPU tensors"
            )

        # resolved page format of the fp8 and fp4 modes ("bfloat16" |
        # "float16" | "float8_e4m3fn")
        self.kv_dtype = resolve_kv_dtype(
            groups, config.kv_dtype, fp8=config.serialize != "raw")
        check_serialize_kv_dtype(config.serialize, self.kv_dtype)

        native_groups = []
        self.group_geometry: List[dict] = []
        max_file_bytes = 0
        max_device_bytes = 0
        for gi, g in enumerate(groups):
            ptrs = [t.data_ptr() for t in g]
            strides = [t.stride(0) * t.element_size() for t in g]
            block_bytes = {t.stride(0) * t.element_size() for t in g}
            if len(block_bytes) != 1:
                raise ValueError("all layers of a group must share block_bytes")
            bb = block_bytes.pop()
            # the actual payload per block may be smaller than the stride;
            # canonical layouts are dense so stride == payload
            native_groups.append((ptrs, strides, bb, int(g[0].shape[0])))
            footer = CHECKSUM_FOOTER_BYTES if config.checksum else 0
            if config.serialize in ("fp8_e4m3_group", "fp4_e2m1_group"):
                record_bytes = tile_record_bytes(
                    config.serialize, bb, config.fp8_group_size, gi,
                    config.checksum, config.fp4_group_size,
                    kv_dtype=self.kv_dtype)
            else:
                record_bytes = footer + (
                    bb // 2 + 4 if config.serialize == "fp8_e4m3" else bb)
            self.group_geometry.append(
                {
                    "num_layers": len(g),
                    "block_bytes": bb,
                    "record_bytes": record_bytes,
                    "num_device_blocks": g[0].shape[0],
                }
            )
            # mirrors the native engine's staging sizes: raw block_bytes per
            # tile, or with footers the real record stride and, behind the
            # device bounce, the seal/verify scratch (8 bytes per workgroup,
            # at most tiles + 2048 of them)
            tiles = config.gpu_blocks_per_file * len(g)
            if config.checksum:
                fb = tiles * record_bytes
                max_file_bytes = max(max_file_bytes, fb)
                max_device_bytes = max(
                    max_device_bytes, (fb + 15) // 16 * 16 + (tiles + 2048) * 8)
            else:
                max_file_bytes = max(max_file_bytes, tiles * bb)
                max_device_bytes = max_file_bytes

        # staging budget clamp: per worker we allocate host staging (and in
        # staged mode a device bounce)
        per_thread = max_file_bytes + (
            max_device_bytes if config.copy_path == "staged" else 0)
        io_threads = config.io_threads
        if per_thread > 0:
            budget_threads = max(1, config.staging_budget_bytes // per_thread)
            io_threads = min(io_threads, budget_threads)

        stream = 0
        if gpu_mode:
            torch.cuda.init()
        self.gpu_mode = gpu_mode
        self._engine = self._ko.StorageOffloadEngine(
            native_groups,
            io_threads=int(io_threads),
            gpu_blocks_per_file=config.gpu_blocks_per_file,
            read_preferring_ratio=config.read_preferring_ratio,
            max_write_queued_seconds=config.max_write_queued_seconds,
            gpu_mode=gpu_mode,
            device=config.device,
            copy_path=config.copy_path,
            serialize=config.serialize,
            host_cache_bytes=config.host_cache_bytes,
            write_policy=config.write_policy,
            direct_io=config.direct_io,
            fp8_group_size=config.fp8_group_size,
            checksum=config.checksum,
            kv_dtype=self.kv_dtype,
            fp4_group_size=config.fp4_group_size,
        )
        del stream
        # keep tensor refs: the native engine holds raw pointers
        self._tensors = [list(g) for g in groups]
        import threading

        self._fin_lock = threading.Lock()
        self._fin_buffer = {}

    @property
    def native(self):
        return self._engine

    def current_stream_handle(self) -> int:
        if not self.gpu_mode:
            return 0
        import torch

        return torch.cuda.current_stream().cuda_stream

    def async_store(self, files, stream: int = None) -> int:
        if stream is None:
            stream = self.current_stream_handle()
        return self._engine.async_store(files, stream)

    def async_load(self, files) -> int:
        return self._engine.async_load(files)

    def get_finished(self):
        return self._engine.get_finished()

    def poll_finished(self, job_ids):
        """Drain engine completions into a shared buffer and pop the ones in
        job_ids — several handlers can share one engine without stealing
        each other's completions."""
        with self._fin_lock:
            for jid, success, dropped in self._engine.get_finished():
                self._fin_buffer[jid] = (success, dropped)
            out = []
            for jid in list(job_ids):
                if jid in self._fin_buffer:
                    success, dropped = self._fin_buffer.pop(jid)
                    out.append((jid, success, dropped))
            return out

    def wait_job(self, job_id: int) -> bool:
        return self._engine.wait_job(job_id)

    def cancel_job(self, job_id: int) -> bool:
        """Non-blocking cancel: queued tasks bail when dequeued. Set flags
        for every job being preempted first, then wait_job each."""
        return self._engine.cancel_job(job_id)

    def stats(self):
        return self._engine.stats()

    def dram_chunk(self, path: str, n_blocks: int, group: int = 0):
        """Read a chunk file's payload out of the pinned host-DRAM cache
        (peer/DRAM-tier bridge). Returns a host uint8 tensor of exactly the
        first n_blocks' packed bytes, or None on a cache miss / short
        entry. The payload layout matches the file layout (raw gather
        layout, per-tile fp8 records when serialize="fp8_e4m3", group-scaled
        fp8 records when serialize="fp8_e4m3_group", group-scaled fp4
        records when serialize="fp4_e2m1_group"). With checksum=True
        every record in the returned slab still carries its 16-byte footer
        (record stride = group_geometry[group]["record_bytes"]); the slab is
        handed out as stored, it is not verified here."""
        import torch

        geo = self.group_geometry[group]
        want = n_blocks * geo["num_layers"] * geo["record_bytes"]
        cap = (self.config.gpu_blocks_per_file * geo["num_layers"]
               * geo["record_bytes"])
        buf = torch.empty(cap, dtype=torch.uint8)
        got = self._engine.host_cache_read(path, buf.data_ptr(), cap)
        if got < want:
            return None
        return buf[:want]
