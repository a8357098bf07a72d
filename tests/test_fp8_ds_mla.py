"""serialize="fp8_ds_mla" on the host path: per 576-element token row the 512
latent values go to e4m3 with one f32 scale per 128, the 64 RoPE values are
kept bit for bit; 656 bytes per row.

Everything is byte equality against a few lines of torch: the latent part is
the fp8_e4m3_group oracle at G = 128 on x[..., :512], the tail is the source
bytes. The tail holds random 16-bit patterns (NaN, Inf, subnormals), so a
tail that is converted instead of copied fails. test_fp8_ds_mla_gpu.py holds
the HIP kernels to the same bytes with the helpers below.
"""
import pytest
import torch

import checksum_oracle
import fp8_fp16_oracle
import fp8_group_oracle
from fp8_group_oracle import wait_finished
from llm_d_kv_cache_amd.offload import (
    FileMapper,
    GPUToStorageHandler,
    KVCacheLayoutConfig,
    OffloadEngineConfig,
    StorageToGPUHandler,
    TorchOffloadEngine,
    tile_record_bytes,
)

_cases = {}


def mla_case(rows, nl, nb, dtype=torch.bfloat16):
    """(pages, ids, file bytes, loaded int16 bits per layer), computed once
    per shape and read-only. Pages hold 2*nb+2 blocks of rows*576 elements:
    latent randn with each 128-run scaled by 10**U(-3, 2) and one all-zero
    run per tile, tail random 16-bit patterns; ids are the nb odd blocks."""
    key = (rows, nl, nb, dtype)
    if key in _cases:
        return _cases[key]
    gen = torch.Generator().manual_seed(rows * 1000 + nl + nb)
    oracle = (fp8_fp16_oracle if dtype == torch.float16
              else fp8_group_oracle).oracle
    blocks, ids = 2 * nb + 2, list(range(1, 2 * nb, 2))
    b = torch.arange(blocks)
    pages, recs, loaded = [], [], []
    for _ in range(nl):
        lat = torch.randn(blocks, rows * 4, 128, generator=gen)
        lat *= 10.0 ** (torch.rand(blocks, rows * 4, 1, generator=gen) * 5 - 3)
        lat[b, b % (rows * 4)] = 0.0
        lat = lat.reshape(blocks, rows, 512).to(dtype)
        tail = (torch.randint(0, 65536, (blocks, rows, 64), generator=gen)
                - 32768).to(torch.int16)
        pages.append(torch.cat([lat.view(torch.int16), tail], -1)
                     .reshape(blocks, rows * 576).view(dtype))
        q, scale, y, _ = oracle(lat[ids], 128)
        recs.append(torch.cat([q, scale.contiguous().view(torch.uint8),
                               tail[ids].contiguous().view(torch.uint8)], -1))
        loaded.append(torch.cat([y.view(torch.int16), tail[ids]], -1)
                      .reshape(nb, rows * 576))
    _cases[key] = (pages, ids, torch.stack(recs, 1).reshape(-1), loaded)
    return _cases[key]


def mla_engine(pages, tmp, nb, copy_path, **kw):
    eng = TorchOffloadEngine(
        [pages], OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=nb,
                                     copy_path=copy_path,
                                     serialize="fp8_ds_mla", **kw))
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(
        model="mla", dtype="bfloat16+fp8mla"))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [nb]),
            StorageToGPUHandler(eng, mapper, [nb]))


def assert_loaded(pages, ids, loaded):
    """Moved blocks hold the reference bits, the others stayed zero."""
    others = [i for i in range(pages[0].shape[0]) if i not in set(ids)]
    for page, want in zip(pages, loaded):
        got = page.cpu().view(torch.int16)
        assert torch.equal(got[ids], want)
        assert (got[others] == 0).all()


def roundtrip(pages, tmp, case, copy_path, **kw):
    """Store the case's odd blocks from `pages` (CPU or GPU copies of the
    input), compare the file, zero the pages, load, compare the bits."""
    src, ids, want, loaded = case
    rows = src[0].shape[1] // 576
    eng, mapper, store, load = mla_engine(pages, tmp, len(ids), copy_path, **kw)
    assert eng.group_geometry[0]["record_bytes"] == \
        656 * rows + 16 * bool(kw.get("checksum"))
    store.transfer_async([0xD5], {0: ids})
    assert wait_finished(store)[0].success
    want = bytes(want.numpy())
    if kw.get("checksum"):
        want = checksum_oracle.seal(want, 656 * rows)
    assert open(mapper.file_name(0xD5, 0), "rb").read() == want, \
        "file bytes differ from the reference"
    for p in pages:
        p.zero_()
    if pages[0].is_cuda:
        torch.cuda.synchronize()  # the engine's streams do not follow torch's
    load.transfer_async([0xD5], {0: ids})
    assert wait_finished(load)[0].success
    assert_loaded(pages, ids, loaded)


@pytest.mark.parametrize("rows,dtype,checksum", [
    (1, torch.bfloat16, False), (5, torch.bfloat16, True),
    (16, torch.bfloat16, False), (1, torch.float16, False),
    (5, torch.float16, False), (16, torch.float16, True)])
def test_host_roundtrip_matches_reference(tmp_path, rows, dtype, checksum):
    case = mla_case(rows, 2, 4, dtype)
    roundtrip([p.clone() for p in case[0]], tmp_path, case, "host",
              checksum=checksum)


def copier_roundtrip(pages, case):
    """BlockCopier gather/scatter, the methods the object tier rides, on the
    torch current stream; a guard band behind the slab catches a store past
    the last entry."""
    from llm_d_kv_cache_amd.ops import block_copier

    _, ids, want, loaded = case
    copier = block_copier([pages])
    n = copier.packed_bytes_fp8_mla(0, len(ids))
    assert n == want.numel()
    slab = torch.full((n + 256,), 0xA5, dtype=torch.uint8,
                      device=pages[0].device)
    stream = (torch.cuda.current_stream().cuda_stream
              if pages[0].is_cuda else 0)
    copier.gather_fp8_mla(0, ids, slab.data_ptr(), stream)
    host = slab.cpu()
    assert torch.equal(host[:n], want) and (host[n:] == 0xA5).all()
    for p in pages:
        p.zero_()
    copier.scatter_fp8_mla(0, ids, slab.data_ptr(), stream)
    assert_loaded(pages, ids, loaded)


def test_host_block_copier_matches_reference():
    case = mla_case(5, 2, 4)
    copier_roundtrip([p.clone() for p in case[0]], case)


def test_tile_record_bytes():
    assert tile_record_bytes("fp8_ds_mla", 1152, 128) == 656
    assert tile_record_bytes("fp8_ds_mla", 18432, 64, checksum=True) == \
        16 * 656 + 16
    assert tile_record_bytes("fp8_ds_mla", 5 * 1152, 128,
                             kv_dtype="float16") == 5 * 656


@pytest.mark.parametrize("block_bytes,kv_dtype", [
    (1024, "bfloat16"), (1152 + 16, "bfloat16"), (1152, "float8_e4m3fn")])
def test_rejects_other_rows_and_fp8_pages(block_bytes, kv_dtype):
    with pytest.raises(ValueError):
        tile_record_bytes("fp8_ds_mla", block_bytes, 128, kv_dtype=kv_dtype)
    pages = [torch.zeros(4, block_bytes, dtype=torch.uint8)]
    with pytest.raises(ValueError):
        TorchOffloadEngine([pages], OffloadEngineConfig(
            copy_path="host", serialize="fp8_ds_mla", kv_dtype=kv_dtype))
