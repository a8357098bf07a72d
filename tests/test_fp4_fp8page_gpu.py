"""serialize="fp4_e2m1_group" over fp8 pages (kv_dtype="float8_e4m3fn")
through the HIP kernels on MI355X.

kvc_gather_fp4_group_fp8page / kvc_scatter_fp4_group_fp8page must write and
read exactly the bytes of the CPU oracle (fp4_fp8page_oracle.py), the same
bytes host mode writes (test_fp4_fp8page.py). The kernels map 16 page bytes
to a lane (a group is G/16 = 1..8 lanes); the shapes are the smallest at
which they can still go wrong, (block_bytes, layers, blocks):

  (32, 3, 5)      G=32 and G=16: 20- and 24-byte records, two vectors per
                  tile, the 8-byte code accesses at 4 mod 8
  (1152, 2, 8)    G=128: 72 vectors, a partly filled wave
  (8320, 2, 6)    G=128 and G=16: 520 vectors, three slices per tile, the
                  last one holding one 8-lane group or eight 1-lane groups
  (768, 2, 160)   ids through the device id buffer instead of the kernarg
  (8448, 8, 128)  G=128: 1024 tiles, 2 slices of 256 lanes for 528 vectors,
                  a second grid-stride trip with 16 live lanes
  (2048, 2, 4)    every group width (1/2/4/8 lanes)

Every slab has a guard band behind it, and one test runs layers whose block
stride is larger than block_bytes. No test depends on how a kernel converts,
only on the bytes.
"""
import os

import pytest
import torch

from fp4_fp8page_oracle import (
    EXHAUSTIVE_TILE_BYTES,
    all_codes_slab,
    as_u8,
    assert_bytes,
    assert_group_bound,
    assert_page_bits,
    decode,
    decode_scales,
    exhaustive_page,
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

F8 = torch.float8_e4m3fn

# (block_bytes, group_size, num_layers, blocks == blocks per file)
SHAPES = [
    (32, 32, 3, 5),
    (32, 16, 3, 5),
    (1152, 128, 2, 8),
    (8320, 128, 2, 6),
    (8320, 16, 2, 6),
    (768, 32, 2, 160),
    (8448, 128, 8, 128),
    (2048, 16, 2, 4),
    (2048, 32, 2, 4),
    (2048, 64, 2, 4),
    (2048, 128, 2, 4),
]


def _sid(shape):
    return "bb{}-g{}-l{}-n{}".format(*shape)


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


def to_device(pages):
    """Device copies: returns (the float8 tensors the engine and copier
    get, uint8 views of the same memory for the checks)."""
    views = [p.cuda() for p in pages]
    return views, [as_u8(v) for v in views]


def _clear(backing, block_bytes):
    for buf in backing:
        buf[:, :block_bytes] = 0
    torch.cuda.synchronize()


def _engine(dev_pages, tmp, shape, copy_path, **kw):
    bb, gs, nl, nb = shape
    eng = TorchOffloadEngine(
        [dev_pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=nb,
                            copy_path=copy_path, serialize="fp4_e2m1_group",
                            fp4_group_size=gs, **kw))
    assert eng.kv_dtype == "float8_e4m3fn"
    tag = f"{eng.kv_dtype}+fp4g{gs}" + ("+ck" if kw.get("checksum") else "")
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(
        model=f"gfp4f8-{copy_path}", dtype=tag))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [nb]),
            StorageToGPUHandler(eng, mapper, [nb]))


def _read(path):
    return torch.frombuffer(bytearray(open(path, "rb").read()),
                            dtype=torch.uint8)


def _check_loaded(backing, shape):
    """Loaded blocks equal the oracle's page bytes, every group is within
    REL_BOUND of its own amax, the other blocks stayed zero."""
    bb, gs, nl, nb = shape
    pages, ids, _, deq = cpu_pages(shape)
    others = [i for i in range(2 * nb + 2) if i not in set(ids)]
    for buf, page, y in zip(backing, pages, deq):
        got = buf.cpu()
        assert_page_bits(got[ids, :bb], y, "loaded pages")
        assert_group_bound(got[ids, :bb], page[ids], gs)
        assert (got[others, :bb] == 0).all()


def _engine_roundtrip(tmp_path, shape, copy_path, **kw):
    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages, backing = to_device(pages)
    eng, mapper, store, load = _engine(dev_pages, tmp_path, shape, copy_path,
                                       **kw)
    store.transfer_async([0x71], {0: ids})
    assert wait_finished(store)[0].success
    data = _read(mapper.file_name(0x71, 0))
    _clear(backing, bb)
    load.transfer_async([0x71], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    _check_loaded(backing, shape)
    return eng, data, want


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_gpu_engine_roundtrip_matches_oracle(tmp_path, shape, copy_path):
    bb, gs, nl, nb = shape
    _, data, want = _engine_roundtrip(tmp_path, shape, copy_path)
    assert data.numel() == nb * nl * record_bytes(bb, gs)
    assert_bytes(data, want, "file")


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] <= 128],
                         ids=_sid)
def test_gpu_block_copier_matches_oracle(shape):
    """BlockCopier.gather_fp4_group / scatter_fp4_group on device."""
    from llm_d_kv_cache_amd.ops import block_copier

    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages, backing = to_device(pages)
    copier = block_copier([dev_pages])
    nbytes = copier.packed_bytes_fp4_group(0, len(ids), gs)
    assert nbytes == want.numel()
    # a guard band behind the slab catches a store past the last record
    slab = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    copier.gather_fp4_group(0, ids, slab.data_ptr(), gs, stream)
    torch.cuda.synchronize()
    host = slab.cpu()
    assert_bytes(host[:nbytes], want, "slab")
    assert (host[nbytes:] == 0xA5).all()
    _clear(backing, bb)
    copier.scatter_fp4_group(0, ids, slab.data_ptr(), gs, stream)
    torch.cuda.synchronize()
    _check_loaded(backing, shape)


def test_gpu_strided_layers():
    """Per-layer strides that differ and exceed block_bytes: layer 0 is
    contiguous, layer 1 a view whose rows are block_bytes + 48 bytes apart
    with 0x5A in the padding. Block ids out of order with a gap. The slab
    equals the oracle and no scatter touches the padding."""
    from llm_d_kv_cache_amd import ensure_offload_native

    ko = ensure_offload_native()
    bb, gs, pad, nblk = 1152, 128, 48, 12
    ids = [9, 2, 7, 4]
    others = [i for i in range(nblk) if i not in ids]
    pages = make_pages(nblk, bb, gs, 2, seed=33)
    flat = as_u8(pages[0]).cuda()
    base = torch.full((nblk, bb + pad), 0x5A, dtype=torch.uint8, device="cuda")
    base[:, :bb] = as_u8(pages[1]).cuda()
    copier = ko.BlockCopier(
        [([flat.data_ptr(), base.data_ptr()], [bb, bb + pad], bb, nblk)],
        gpu_mode=True, kv_dtype="float8_e4m3fn")
    stream = torch.cuda.current_stream().cuda_stream
    want = oracle_records(pages, ids, gs)
    nbytes = copier.packed_bytes_fp4_group(0, len(ids), gs)
    assert nbytes == want.numel()
    slab = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    copier.gather_fp4_group(0, ids, slab.data_ptr(), gs, stream)
    torch.cuda.synchronize()
    host = slab.cpu()
    assert_bytes(host[:nbytes], want, "slab")
    assert (host[nbytes:] == 0xA5).all(), "guard band overwritten"
    flat.zero_()
    base[:, :bb] = 0
    torch.cuda.synchronize()
    copier.scatter_fp4_group(0, ids, slab.data_ptr(), gs, stream)
    torch.cuda.synchronize()
    for got, page in zip((flat.cpu(), base[:, :bb].cpu()), pages):
        assert_page_bits(got[ids], oracle(page[ids], gs)[2], "scattered")
        assert (got[others] == 0).all()
    assert (base[:, bb:] == 0x5A).all(), "padding overwritten"


def test_gpu_scatter_of_every_code_byte():
    """A hand-built slab holding all 256 code bytes under each of the 126
    scales an encoder can write, against the oracle decode."""
    from llm_d_kv_cache_amd.ops import block_copier

    scales = decode_scales()
    slab, codes, scale = all_codes_slab(scales)
    tiles = scales.numel()
    page = torch.zeros(tiles + 1, 512, dtype=torch.uint8, device="cuda")
    copier = block_copier([[page.view(F8)]])
    dev = torch.cat([slab, torch.full((256,), 0xA5, dtype=torch.uint8)]).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    copier.scatter_fp4_group(0, list(range(tiles)), dev.data_ptr(), 16, stream)
    torch.cuda.synchronize()
    got = page.cpu()
    want = decode(codes.reshape(tiles, 32, 16), scale[..., None])
    assert_page_bits(got[:tiles], want.reshape(tiles, 512), "decoded slab")
    assert (got[:tiles, 2 * 0x80 + 1] == 0x80).all()  # -0.0 stays -0.0
    assert (got[tiles] == 0).all()


def test_gpu_exhaustive_page():
    """Every finite x under every amax >= |x| (fp4_fp8page_oracle.
    exhaustive_page, the input of the host-mode exhaustive test), through
    the device gather and scatter."""
    from llm_d_kv_cache_amd.ops import block_copier

    page = exhaustive_page()
    blocks = page.shape[0]
    ids = list(range(blocks))
    want = oracle_records([page], ids, 16)
    y = oracle(page, 16)[2]
    dev_page = page.cuda()
    copier = block_copier([[dev_page.view(F8)]])
    rec = record_bytes(EXHAUSTIVE_TILE_BYTES, 16)
    slab = torch.full((blocks * rec + 256,), 0xA5, dtype=torch.uint8,
                      device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    copier.gather_fp4_group(0, ids, slab.data_ptr(), 16, stream)
    torch.cuda.synchronize()
    host = slab.cpu()
    assert_bytes(host[:blocks * rec], want, "slab")
    assert (host[blocks * rec:] == 0xA5).all()
    dev_page.zero_()
    copier.scatter_fp4_group(0, ids, slab.data_ptr(), 16, stream)
    torch.cuda.synchronize()
    assert_page_bits(dev_page.cpu(), y, "round trip")
    assert_group_bound(dev_page.cpu(), page, 16)


def test_gpu_file_equals_host_mode_file(tmp_path):
    """The same general input through a GPU engine and a host-mode engine:
    byte-identical files, and each loads the other's."""
    shape = (8320, 128, 2, 6)
    bb, gs, nl, nb = shape
    pages, ids, want, deq = cpu_pages(shape)
    _, data, _ = _engine_roundtrip(tmp_path / "gpu", shape, "staged")
    host_pages = [p.clone() for p in pages]
    heng = TorchOffloadEngine(
        [host_pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=nb,
                            copy_path="host", serialize="fp4_e2m1_group",
                            fp4_group_size=gs))
    # same mapper as the GPU engine's: the host engine reads the GPU's file
    mapper = FileMapper(str(tmp_path / "gpu"), KVCacheLayoutConfig(
        model="gfp4f8-staged", dtype=f"float8_e4m3fn+fp4g{gs}"))
    for p in host_pages:
        as_u8(p).zero_()
    load = StorageToGPUHandler(heng, mapper, [nb])
    load.transfer_async([0x71], {0: ids})
    assert wait_finished(load)[0].success
    for p, y in zip(host_pages, deq):
        assert_page_bits(p[ids], y, "host load of the GPU-written file")
    # and the host-mode file
    for p, o in zip(host_pages, pages):
        p.copy_(o)
    hmapper = FileMapper(str(tmp_path / "host"), KVCacheLayoutConfig(
        model="hfp4f8", dtype=f"float8_e4m3fn+fp4g{gs}"))
    store = GPUToStorageHandler(heng, hmapper, [nb])
    store.transfer_async([0x71], {0: ids})
    assert wait_finished(store)[0].success
    assert_bytes(data, _read(hmapper.file_name(0x71, 0)),
                 "GPU-written file against the host-mode file")


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
def test_gpu_checksum_composes(tmp_path, copy_path):
    """checksum=True: payloads are the oracle's bytes, every footer
    verifies, the load passes verification and restores the pages. 24-byte
    payloads: records of 40 bytes."""
    from llm_d_kv_cache_amd.ops import block_copier

    for shape in ((32, 16, 3, 5), (8320, 128, 2, 6)):
        bb, gs, nl, nb = shape
        eng, data, want = _engine_roundtrip(
            tmp_path / f"bb{bb}", shape, copy_path, checksum=True)
        payload = record_bytes(bb, gs)
        tiles = nb * nl
        assert eng.group_geometry[0]["record_bytes"] == payload + 16
        assert data.numel() == tiles * (payload + 16)
        assert_bytes(
            data.reshape(tiles, payload + 16)[:, :payload].reshape(-1),
            want, "payloads")
        host_copier = block_copier([[torch.zeros(1, bb, dtype=torch.uint8)]])
        assert host_copier.verify_records(data.data_ptr(), tiles, payload,
                                          0) == (0, -1)
        st = eng.stats()
        assert st.checksum_failures == 0 and st.errors == 0


def test_gpu_partial_load_with_skip(tmp_path):
    """24 blocks at 16 per file, then blocks 20-23 with
    skip_leading_blocks=20: the tail seek runs on the fp8-page record
    size."""
    bb, gs, nl = 1152, 128, 2
    pages = make_pages(32, bb, gs, nl, seed=21)
    dev_pages, backing = to_device(pages)
    eng, mapper, store, load = _engine(dev_pages, tmp_path, (bb, gs, nl, 16),
                                       "staged")
    store.transfer_async([0xB1, 0xB2], {0: list(range(24))})
    assert wait_finished(store)[0].success
    assert os.path.getsize(mapper.file_name(0xB2, 0)) == \
        8 * nl * record_bytes(bb, gs)
    _clear(backing, bb)
    load.transfer_async([0xB1, 0xB2], {0: list(range(20, 24))},
                        skip_leading_blocks=20)
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    for buf, page in zip(backing, pages):
        got = buf.cpu()
        assert_page_bits(got[20:24, :bb], oracle(page[20:24], gs)[2],
                         "tail blocks")
        assert (got[:20, :bb] == 0).all()
        assert (got[24:, :bb] == 0).all()


def test_gpu_dram_tier_hit_after_file_deleted(tmp_path):
    """Staged path + pinned DRAM tier: the load is served from the resident
    fp4 slab (file deleted to prove it) and dequantized on device."""
    shape = (1152, 128, 2, 8)
    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages, backing = to_device(pages)
    eng, mapper, store, load = _engine(dev_pages, tmp_path, shape, "staged",
                                       host_cache_bytes=8 << 20)
    store.transfer_async([0xCA], {0: ids})
    assert wait_finished(store)[0].success
    assert eng.stats().host_cache_stores == 1
    resident = eng.dram_chunk(mapper.file_name(0xCA, 0), nb, 0)
    assert_bytes(resident, want, "DRAM slab")
    os.unlink(mapper.file_name(0xCA, 0))
    _clear(backing, bb)
    load.transfer_async([0xCA], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    assert eng.stats().host_cache_hits == 1
    _check_loaded(backing, shape)


def test_gpu_fp8_launchers_refuse_fp8_pages():
    """The fp8 methods of a device copier over fp8 pages raise and write
    nothing."""
    from llm_d_kv_cache_amd.ops import block_copier

    page = torch.zeros(4, 2048, dtype=torch.uint8, device="cuda")
    copier = block_copier([[page.view(F8)]])
    slab = torch.full((8192,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for call in (lambda: copier.gather_fp8(0, [0], slab.data_ptr(),
                                           slab.data_ptr() + 4096, stream),
                 lambda: copier.scatter_fp8(0, [0], slab.data_ptr(), stream),
                 lambda: copier.gather_fp8_group(0, [0], slab.data_ptr(), 128,
                                                 stream),
                 lambda: copier.scatter_fp8_group(0, [0], slab.data_ptr(),
                                                  128, stream)):
        with pytest.raises(ValueError, match="already are fp8"):
            call()
    torch.cuda.synchronize()
    assert (slab.cpu() == 0xA5).all() and (page.cpu() == 0).all()
