"""Hot-op kernel API: direct access to the CDNA4 kernels the data plane is
built from, for embedding in other MI355X services.

- gather/scatter: paged KV pages <-> contiguous slabs at the HBM roof
  (BlockCopier; see csrc/offload/kernels.hip).
- prefix_hash: batched chained block hashing on device token buffers
  (one lane per sequence).
- fp8 serialize: quantizing gather / dequantizing scatter are methods on
  the copier (gather_fp8 / scatter_fp8 with packed_bytes_fp8 /
  fp8_scratch_bytes sizing); the offload engine's serialize="fp8_e4m3"
  rides the same kernels.
- group-scaled fp8: gather_fp8_group / scatter_fp8_group (sized by
  packed_bytes_fp8_group) keep one f32 scale per group_size elements
  (64/128/256/512; set it to head_dim) instead of one per tile. The gather
  is a single pass — the group amax is an in-wave butterfly — and needs no
  scratch. serialize="fp8_e4m3_group" rides these kernels.
- group-scaled fp4: gather_fp4_group / scatter_fp4_group (sized by
  packed_bytes_fp4_group) write OCP e2m1 codes, two per byte, with one f32
  scale per group_size elements (16/32/64/128, default 32): records of
  n/2 + 4n/G bytes, a quarter to a third of the bf16 page. Same single-pass
  shape as the fp8-group pair, no scratch. Lossy at 4 bits; the effect on
  model quality has not been measured. serialize="fp4_e2m1_group" rides
  these kernels.
- page format: the fp8 families and the fp4 pair convert bf16 or fp16 pages. The copier is
  built for one format (block_copier(..., kv_dtype="auto"): float16 if
  every page tensor is torch.float16, else bfloat16; pass "float16" /
  "bfloat16" for opaque uint8 views) and every fp8/fp4 method follows it. The
  records are format-free, so the two ends of a transfer need not agree.
- fp8 pages: a copier over torch.float8_e4m3fn tensors (or uint8 views with
  kv_dtype="float8_e4m3fn") has the raw and the fp4 methods. A tile then
  holds block_bytes elements, 16 per lane in the kernels, and an fp4 record
  is block_bytes/2 + 4*block_bytes/G bytes; loads round to e4m3fn. The
  *_fp8 and *_fp8_group methods raise ValueError on such a copier.
- record checksums: packed_bytes*/gather*/scatter* take checksum=True to
  leave a 16-byte footer behind every record; seal_records(ptr, tiles,
  payload_bytes, stream) fills the footers of such a slab and
  verify_records(...) returns (bad records, first bad index or -1).
  record_checksum(buffer) is the host twin of the sum, for tools and tests.
"""
from __future__ import annotations

from typing import List, Optional, Sequence


def block_copier(groups: Sequence[Sequence], device: Optional[int] = None,
                 kv_dtype: str = "auto"):
    """BlockCopier over torch page tensors (GPU or CPU twins).

    kv_dtype (auto | bfloat16 | float16 | float8_e4m3fn) is the page format
    every fp8 and fp4 method of the copier converts with; see
    offload.engine.resolve_kv_dtype."""
    from .. import ensure_offload_native
    from ..offload.engine import resolve_kv_dtype

    ko = ensure_offload_native()
    gpu = groups[0][0].is_cuda
    native = [
        ([t.data_ptr() for t in g],
         [t.stride(0) * t.element_size() for t in g],
         g[0].stride(0) * g[0].element_size(),
         int(g[0].shape[0]))
        for g in groups
    ]
    dev = device if device is not None else (
        groups[0][0].device.index or 0 if gpu else 0)
    return ko.BlockCopier(native, gpu, dev,
                          kv_dtype=resolve_kv_dtype(groups, kv_dtype))


def record_checksum(buffer) -> int:
    """Host twin of the seal/verify kernels' per-record sum (see
    offload.engine.record_checksum)."""
    from ..offload.engine import record_checksum as _rc

    return _rc(buffer)


def prefix_hash(tokens, seq_offsets, seeds, block_size: int = 16,
                stream: Optional[int] = None) -> List[List[int]]:
    """Batched chained block hashing on the GPU.

    tokens: int32 CUDA tensor (flat); seq_offsets: int64 CUDA tensor
    [n_seq+1]; seeds: int64 CUDA tensor [n_seq] (chain seeds, two's
    complement of the uint64 parent/model hash). Returns per-sequence key
    lists (uint64 as Python ints). Must match TokenProcessor bit-exactly
    (tested in tests/test_offload_gpu.py).
    """
    import torch

    from .. import ensure_offload_native

    ko = ensure_offload_native()
    n_seq = seeds.numel()
    lens = (seq_offsets[1:] - seq_offsets[:-1]) // block_size
    key_off = torch.zeros(n_seq + 1, dtype=torch.int64, device=tokens.device)
    torch.cumsum(lens, 0, out=key_off[1:])
    keys = torch.zeros(int(key_off[-1].item()), dtype=torch.int64,
                       device=tokens.device)
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    ko.prefix_hash(tokens.data_ptr(), seq_offsets.data_ptr(), seeds.data_ptr(),
                   keys.data_ptr(), key_off.data_ptr(), block_size, n_seq,
                   stream)
    torch.cuda.synchronize()
    off = key_off.cpu().tolist()
    vals = keys.cpu().numpy().astype("uint64").tolist()
    return [vals[off[i]:off[i + 1]] for i in range(n_seq)]
