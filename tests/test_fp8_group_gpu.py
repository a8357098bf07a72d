"""serialize="fp8_e4m3_group" through the HIP kernels on MI355X.

kvc_gather_fp8_group / kvc_scatter_fp8_group must write and read exactly
the bytes of the CPU oracle (fp8_group_oracle.py) — the same bytes host
mode writes (test_fp8_group.py) — so files move freely between GPU and
host-mode engines. Shapes are the smallest at which the kernels can still
go wrong:

  768 B tiles   48 vectors: a partly filled wave, one workgroup per tile
  8448 B tiles  528 vectors: three slices per tile, the last one holding
                a single 16-lane group
  64 KiB tiles  every group width (8/16/32/64 lanes), many slices
  160 blocks    ids through the device id buffer instead of the kernarg
  8448 B x 8 x 128   1024 tiles: 2 slices of 256 lanes for 528 vectors, so
                lanes take a second grid-stride trip, on which wave 0 of
                slice 0 re-enters the shuffle with 48 dead lanes
"""
import os

import pytest
import torch

from fp8_group_oracle import (
    assert_group_bound,
    make_pages,
    oracle,
    oracle_records,
    record_bytes,
    wait_finished,
)
from llm_d_kv_cache_amd.offload import (
    FileMapper,
    GPUToStorageHandler,
    KVCacheLayoutConfig,
    OffloadEngineConfig,
    StorageToGPUHandler,
    TorchOffloadEngine,
)

pytestmark = pytest.mark.gpu

# (block_bytes, group_size, num_layers, blocks == blocks per file)
SHAPES = [
    (768, 128, 2, 4),
    (8448, 128, 2, 4),
    (65536, 64, 4, 16),
    (65536, 128, 4, 16),
    (65536, 256, 4, 16),
    (65536, 512, 4, 16),
    (768, 128, 2, 160),
    (8448, 128, 8, 128),
]
SHAPE_IDS = [f"bb{b}-g{g}-l{l}-n{n}" for b, g, l, n in SHAPES]

_inputs = {}


def cpu_pages(shape):
    """CPU pages + per-layer oracle of one shape, computed once and shared
    (read-only) by every test that uses the shape. Pages hold 2n+2 blocks;
    the tests move the n odd ones."""
    if shape not in _inputs:
        bb, gs, nl, nb = shape
        pages = make_pages(2 * nb + 2, bb, gs, nl, seed=bb + gs + nb)
        ids = list(range(1, 2 * nb, 2))
        _inputs[shape] = (pages, ids, oracle_records(pages, ids, gs),
                          [oracle(p[ids], gs)[2] for p in pages])
    return _inputs[shape]


def _engine(dev_pages, tmp, shape, copy_path, **kw):
    bb, gs, nl, nb = shape
    eng = TorchOffloadEngine(
        [dev_pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=nb,
                            copy_path=copy_path, serialize="fp8_e4m3_group",
                            fp8_group_size=gs, **kw))
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(
        model=f"gfp8g-{copy_path}", dtype=f"bfloat16+fp8g{gs}"))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [nb]),
            StorageToGPUHandler(eng, mapper, [nb]))


def _check_loaded(dev_pages, shape):
    """Loaded blocks equal the oracle's dequantized values bit for bit,
    every group is within 0.07 of its own amax, the rest stayed zero."""
    bb, gs, nl, nb = shape
    pages, ids, _, deq = cpu_pages(shape)
    others = [i for i in range(2 * nb + 2) if i not in set(ids)]
    for dev, page, y in zip(dev_pages, pages, deq):
        got = dev.cpu()
        assert torch.equal(got[ids].view(torch.int16), y.view(torch.int16))
        assert_group_bound(got[ids], page[ids], gs)
        assert (got[others].view(torch.int16) == 0).all()


def _assert_bytes(got, want, what):
    assert got.numel() == want.numel(), \
        f"{what}: {got.numel()} bytes, oracle has {want.numel()}"
    diff = (got != want).nonzero().flatten()
    assert diff.numel() == 0, (
        f"{what}: {diff.numel()} bytes differ from the CPU oracle, "
        f"first offsets {diff[:8].tolist()}")


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_gpu_engine_roundtrip_matches_oracle(tmp_path, shape, copy_path):
    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(dev_pages, tmp_path, shape, copy_path)
    store.transfer_async([0x71], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0x71, 0)
    assert os.path.getsize(path) == nb * nl * record_bytes(bb, gs)
    data = torch.frombuffer(bytearray(open(path, "rb").read()),
                            dtype=torch.uint8)
    _assert_bytes(data, want, "file")
    for t in dev_pages:
        t.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0x71], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    _check_loaded(dev_pages, shape)


@pytest.mark.parametrize("shape", SHAPES[:6] + SHAPES[7:],
                         ids=SHAPE_IDS[:6] + SHAPE_IDS[7:])
def test_gpu_block_copier_matches_oracle(shape):
    """BlockCopier.gather_fp8_group / scatter_fp8_group on device."""
    from llm_d_kv_cache_amd.ops import block_copier

    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    copier = block_copier([dev_pages])
    nbytes = copier.packed_bytes_fp8_group(0, len(ids), gs)
    assert nbytes == want.numel()
    # a guard band behind the slab catches a store past the last record
    slab = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    copier.gather_fp8_group(0, ids, slab.data_ptr(), gs, stream)
    torch.cuda.synchronize()
    host = slab.cpu()
    _assert_bytes(host[:nbytes], want, "slab")
    assert (host[nbytes:] == 0xA5).all()
    for t in dev_pages:
        t.zero_()
    copier.scatter_fp8_group(0, ids, slab.data_ptr(), gs, stream)
    torch.cuda.synchronize()
    _check_loaded(dev_pages, shape)


def test_gpu_partial_load_with_skip(tmp_path):
    """24 blocks at 16 per file, then blocks 20-23 with
    skip_leading_blocks=20: the tail seek runs on grouped record sizes."""
    bb, gs, nl = 8448, 128, 2
    pages = make_pages(32, bb, gs, nl, seed=21)
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(dev_pages, tmp_path, (bb, gs, nl, 16),
                                       "staged")
    store.transfer_async([0xB1, 0xB2], {0: list(range(24))})
    assert wait_finished(store)[0].success
    assert os.path.getsize(mapper.file_name(0xB2, 0)) == \
        8 * nl * record_bytes(bb, gs)
    for t in dev_pages:
        t.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0xB1, 0xB2], {0: list(range(20, 24))},
                        skip_leading_blocks=20)
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    for dev, page in zip(dev_pages, pages):
        got = dev.cpu()
        y = oracle(page[20:24], gs)[2]
        assert torch.equal(got[20:24].view(torch.int16), y.view(torch.int16))
        assert (got[:20].view(torch.int16) == 0).all()
        assert (got[24:].view(torch.int16) == 0).all()


def test_gpu_dram_tier_hit_after_file_deleted(tmp_path):
    """Staged path + pinned DRAM tier: the load is served from the resident
    grouped slab (file deleted to prove it) and dequantized on device."""
    shape = SHAPES[0]
    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(dev_pages, tmp_path, shape, "staged",
                                       host_cache_bytes=8 << 20)
    store.transfer_async([0xCA], {0: ids})
    assert wait_finished(store)[0].success
    assert eng.stats().host_cache_stores == 1
    resident = eng.dram_chunk(mapper.file_name(0xCA, 0), nb, 0)
    _assert_bytes(resident, want, "DRAM slab")
    os.unlink(mapper.file_name(0xCA, 0))
    for t in dev_pages:
        t.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0xCA], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    assert eng.stats().host_cache_hits == 1
    _check_loaded(dev_pages, shape)
