"""serialize="fp8_e4m3" (one f32 scale per tile) through the HIP kernels on
MI355X, byte for byte against the CPU oracle (fp8_tile_oracle.py).

The staged path runs the split gather (kvc_fp8_amax + kvc_fp8_quant), the
zero-copy path the fused one (kvc_gather_fp8), loads run kvc_scatter_fp8;
all are held to the same bytes, the bytes host mode writes too
(test_fp8_tile.py), so the split and the fused gather are thereby equal to
each other and files move freely between GPU and host-mode engines. The
input plants every tile's maximum where a reduction could lose it (see
fp8_tile_oracle.positions). Shapes, (block_bytes, layers, blocks):

  (16, 3, 5)      one vector per tile: 63 dead lanes, three dead waves; the
                  record is 12 bytes, so the dwordx2 stores of odd tiles
                  sit at 4 mod 8 (BlockCopier only)
  (1152, 2, 8)    72 vectors: wave 1 partly filled, waves 2-3 idle
  (8208, 2, 6)    513 vectors, 3 slices, the last one holding one vector —
                  and the last planted maximum
  (768, 2, 160)   ids through the device id buffer (engine only)
  (8448, 8, 128)  1024 tiles: 2 slices of 256 lanes for 528 vectors, a
                  second grid-stride trip (three in the fused kernel)
"""
import os

import pytest
import torch

from fp8_tile_oracle import (
    assert_tile_bound,
    make_tile_pages,
    record_bytes,
    tile_oracle,
    tile_records,
    tile_values,
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

S16 = (16, 3, 5)
S1152 = (1152, 2, 8)
S8208 = (8208, 2, 6)
S768 = (768, 2, 160)
S8448 = (8448, 8, 128)


def _id(shape):
    return "bb{}-l{}-n{}".format(*shape)


ENGINE_SHAPES = [S1152, S8208, S768, S8448]
COPIER_SHAPES = [S16, S1152, S8208, S8448]

_inputs = {}


def cpu_pages(shape):
    """CPU pages of 2n+2 blocks, the n odd ids the tests move, the oracle's
    record bytes and dequantized values; computed once per shape and shared
    read-only."""
    if shape not in _inputs:
        bb, nl, nb = shape
        pages = make_tile_pages(2 * nb + 2, bb, nl, seed=bb + nl + nb)
        ids = list(range(1, 2 * nb, 2))
        _inputs[shape] = (pages, ids, tile_records(pages, ids),
                          tile_values(pages, ids))
    return _inputs[shape]


def _engine(pages, tmp, shape, copy_path):
    bb, nl, nb = shape
    eng = TorchOffloadEngine(
        [pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=nb,
                            copy_path=copy_path, serialize="fp8_e4m3"))
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(
        model=f"gfp8t-{copy_path}", dtype="bfloat16+fp8_e4m3"))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [nb]),
            StorageToGPUHandler(eng, mapper, [nb]))


def _assert_bytes(got, want, what):
    assert got.numel() == want.numel(), \
        f"{what}: {got.numel()} bytes, expected {want.numel()}"
    diff = (got != want).nonzero().flatten()
    assert diff.numel() == 0, (
        f"{what}: {diff.numel()} of {want.numel()} bytes differ, "
        f"first offsets {diff[:8].tolist()}")


def _check_loaded(dev_pages, shape):
    """Moved blocks equal the oracle's dequantized values bit for bit and
    are within 0.07 of their tile's amax; the other blocks stayed zero."""
    bb, nl, nb = shape
    pages, ids, _, deq = cpu_pages(shape)
    others = [i for i in range(2 * nb + 2) if i not in set(ids)]
    for dev, page, y in zip(dev_pages, pages, deq):
        got = dev.cpu()
        assert torch.equal(got[ids].view(torch.int16), y.view(torch.int16))
        assert_tile_bound(got[ids], page[ids])
        assert (got[others].view(torch.int16) == 0).all()


def _file(path):
    return torch.frombuffer(bytearray(open(path, "rb").read()),
                            dtype=torch.uint8)


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", ENGINE_SHAPES, ids=_id)
def test_gpu_engine_roundtrip_matches_oracle(tmp_path, shape, copy_path):
    bb, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(dev_pages, tmp_path, shape, copy_path)
    store.transfer_async([0x71], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0x71, 0)
    assert os.path.getsize(path) == nb * nl * record_bytes(bb)
    _assert_bytes(_file(path), want, "file/oracle")
    for t in dev_pages:
        t.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0x71], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    _check_loaded(dev_pages, shape)


@pytest.mark.parametrize("shape", COPIER_SHAPES, ids=_id)
def test_gpu_block_copier_matches_oracle(shape):
    """BlockCopier.gather_fp8 (split kernels) / scatter_fp8 on device."""
    from llm_d_kv_cache_amd.ops import block_copier

    bb, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    copier = block_copier([dev_pages])
    nbytes = copier.packed_bytes_fp8(0, len(ids))
    assert nbytes == want.numel()
    scratch = torch.empty(copier.fp8_scratch_bytes(0, len(ids)),
                          dtype=torch.uint8, device="cuda")
    # a guard band behind the slab catches a store past the last record
    slab = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    copier.gather_fp8(0, ids, slab.data_ptr(), scratch.data_ptr(), stream)
    torch.cuda.synchronize()
    host = slab.cpu()
    _assert_bytes(host[:nbytes], want, "slab/oracle")
    assert (host[nbytes:] == 0xA5).all(), "guard band overwritten"
    for t in dev_pages:
        t.zero_()
    copier.scatter_fp8(0, ids, slab.data_ptr(), stream)
    torch.cuda.synchronize()
    _check_loaded(dev_pages, shape)


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", [S1152, S8208], ids=_id)
def test_gpu_file_equals_host_mode_file(tmp_path, shape, copy_path):
    """On general input (ties included) a GPU engine writes byte for byte
    the file a host-mode engine writes for the same pages."""
    pages, ids, want, _ = cpu_pages(shape)
    host_pages = [p.clone() for p in pages]
    _, hm, hstore, _ = _engine(host_pages, tmp_path / "host", shape, "host")
    hstore.transfer_async([0x71], {0: ids})
    assert wait_finished(hstore)[0].success
    host_file = _file(hm.file_name(0x71, 0))

    dev_pages = [p.cuda() for p in pages]
    _, mapper, store, _ = _engine(dev_pages, tmp_path / "gpu", shape,
                                  copy_path)
    store.transfer_async([0x71], {0: ids})
    assert wait_finished(store)[0].success
    _assert_bytes(_file(mapper.file_name(0x71, 0)), host_file,
                  "file/host mode")
    _assert_bytes(host_file, want, "host-mode file/oracle")


def test_gpu_partial_load_with_skip(tmp_path):
    """24 blocks at 16 per file, then blocks 20-23 with
    skip_leading_blocks=20: the tail seek runs on n + 4 byte records."""
    bb, nl = 1152, 2
    pages = make_tile_pages(32, bb, nl, seed=21)
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(dev_pages, tmp_path, (bb, nl, 16),
                                       "staged")
    store.transfer_async([0xB1, 0xB2], {0: list(range(24))})
    assert wait_finished(store)[0].success
    assert os.path.getsize(mapper.file_name(0xB2, 0)) == \
        8 * nl * record_bytes(bb)
    for t in dev_pages:
        t.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0xB1, 0xB2], {0: list(range(20, 24))},
                        skip_leading_blocks=20)
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    for dev, page in zip(dev_pages, pages):
        got = dev.cpu()
        y = tile_oracle(page[20:24])[2]
        assert torch.equal(got[20:24].view(torch.int16), y.view(torch.int16))
        assert (got[:20].view(torch.int16) == 0).all()
        assert (got[24:].view(torch.int16) == 0).all()


def test_gpu_strided_layers_raw_and_fp8():
    """Per-layer strides that differ and exceed block_bytes: layer 0 is
    contiguous, layer 1 a view whose rows are block_bytes + 128 bytes apart
    with 0x5A in the padding. Block ids out of order with a gap. Raw slabs
    equal the plain torch gather, fp8 slabs the oracle, and no scatter
    touches the padding."""
    from llm_d_kv_cache_amd import ensure_offload_native

    ko = ensure_offload_native()
    bb, pad, nblk = 1152, 128, 12
    ids = [9, 2, 7, 4]
    others = [i for i in range(nblk) if i not in ids]
    pages = make_tile_pages(nblk, bb, 2, seed=33)
    flat = pages[0].cuda()
    base = torch.full((nblk, bb + pad), 0x5A, dtype=torch.uint8, device="cuda")
    base[:, :bb] = pages[1].view(torch.uint8).cuda()
    wide = base[:, :bb]                    # row stride bb + pad bytes
    assert wide.stride(0) == bb + pad and wide.data_ptr() == base.data_ptr()
    copier = ko.BlockCopier(
        [([flat.data_ptr(), wide.data_ptr()], [bb, bb + pad], bb, nblk)],
        gpu_mode=True)
    stream = torch.cuda.current_stream().cuda_stream

    def layers_now():
        return [flat.cpu(), base[:, :bb].cpu().contiguous().view(torch.bfloat16)]

    def clear():
        flat.zero_()
        base[:, :bb] = 0
        torch.cuda.synchronize()

    def padding_intact():
        return bool((base[:, bb:] == 0x5A).all())

    # raw
    nraw = copier.packed_bytes(0, len(ids))
    assert nraw == len(ids) * 2 * bb
    slab = torch.full((nraw + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    copier.gather(0, ids, slab.data_ptr(), stream)
    torch.cuda.synchronize()
    ref = torch.cat([p[i].view(torch.uint8) for i in ids for p in pages])
    host = slab.cpu()
    _assert_bytes(host[:nraw], ref, "raw slab/torch gather")
    assert (host[nraw:] == 0xA5).all(), "guard band overwritten"
    clear()
    copier.scatter(0, ids, slab.data_ptr(), stream)
    torch.cuda.synchronize()
    for got, page in zip(layers_now(), pages):
        assert torch.equal(got[ids].view(torch.int16),
                           page[ids].view(torch.int16))
        assert (got[others].view(torch.int16) == 0).all()
    assert padding_intact()

    # per-tile fp8
    flat.copy_(pages[0])
    base[:, :bb] = pages[1].view(torch.uint8).cuda()
    nfp8 = copier.packed_bytes_fp8(0, len(ids))
    want = tile_records(pages, ids)
    assert nfp8 == want.numel()
    scratch = torch.empty(copier.fp8_scratch_bytes(0, len(ids)),
                          dtype=torch.uint8, device="cuda")
    slab = torch.full((nfp8 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    copier.gather_fp8(0, ids, slab.data_ptr(), scratch.data_ptr(), stream)
    torch.cuda.synchronize()
    host = slab.cpu()
    _assert_bytes(host[:nfp8], want, "fp8 slab/oracle")
    assert (host[nfp8:] == 0xA5).all(), "guard band overwritten"
    clear()
    copier.scatter_fp8(0, ids, slab.data_ptr(), stream)
    torch.cuda.synchronize()
    for got, page, y in zip(layers_now(), pages, tile_values(pages, ids)):
        assert torch.equal(got[ids].view(torch.int16), y.view(torch.int16))
        assert_tile_bound(got[ids], page[ids])
        assert (got[others].view(torch.int16) == 0).all()
    assert padding_intact()
