"""serialize="fp4_e2m1_group" through the HIP kernels on MI355X.

kvc_gather_fp4_group / kvc_scatter_fp4_group must write and read exactly
the bytes of the CPU oracle (fp4_group_oracle.py), the same bytes host mode
writes (test_fp4_group.py), so files move freely between GPU and host-mode
engines. The kernels map 8 page values to a lane (a group is G/8 = 2..16
lanes); the shapes are the smallest at which they can still go wrong:

  768 B tiles, G=32    48 vectors: a partly filled wave, one workgroup per
                       tile
  8448 B tiles         528 vectors: three slices per tile, the last one
                       holding a single 16-lane group (G=128) or eight
                       2-lane groups (G=16)
  64 KiB tiles         every group width (2/4/8/16 lanes), many slices
  160 blocks           ids through the device id buffer instead of the
                       kernarg
  8448 B x 8 x 128     1024 tiles: 2 slices of 256 lanes for 528 vectors, so
                       lanes take a second grid-stride trip, on which wave 0
                       of slice 0 re-enters the shuffle with 48 dead lanes

bf16 pages unless a test says fp16. No test depends on how the kernels
convert (compare chain or a hardware instruction): only on the bytes.
"""
import os

import pytest
import torch

from fp4_group_oracle import (
    TIE_TILE_BYTES,
    all_codes_slab,
    assert_bits,
    assert_bytes,
    assert_group_bound,
    decode,
    decode_scales,
    exhaustive_groups,
    make_pages,
    make_tie_page,
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
    (768, 32, 2, 4),
    (8448, 128, 2, 4),
    (8448, 16, 2, 4),
    (65536, 16, 4, 16),
    (65536, 32, 4, 16),
    (65536, 64, 4, 16),
    (65536, 128, 4, 16),
    (768, 32, 2, 160),
    (8448, 128, 8, 128),
]
FP16_SHAPES = [(768, 32, 2, 4), (8448, 128, 2, 4), (65536, 16, 4, 16)]


def _sid(shape):
    return "bb{}-g{}-l{}-n{}".format(*shape)


_inputs = {}


def cpu_pages(shape, dtype=torch.bfloat16):
    """CPU pages + per-layer oracle of one shape, computed once and shared
    (read-only) by every test that uses the shape. Pages hold 2n+2 blocks;
    the tests move the n odd ones."""
    key = (shape, dtype)
    if key not in _inputs:
        bb, gs, nl, nb = shape
        pages = make_pages(2 * nb + 2, bb, gs, nl, seed=bb + gs + nb,
                           dtype=dtype)
        ids = list(range(1, 2 * nb, 2))
        _inputs[key] = (pages, ids, oracle_records(pages, ids, gs),
                        [oracle(p[ids], gs)[2] for p in pages])
    return _inputs[key]


def _engine(dev_pages, tmp, shape, copy_path, **kw):
    bb, gs, nl, nb = shape
    eng = TorchOffloadEngine(
        [dev_pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=nb,
                            copy_path=copy_path, serialize="fp4_e2m1_group",
                            fp4_group_size=gs, **kw))
    tag = f"{eng.kv_dtype}+fp4g{gs}" + ("+ck" if kw.get("checksum") else "")
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(
        model=f"gfp4g-{copy_path}", dtype=tag))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [nb]),
            StorageToGPUHandler(eng, mapper, [nb]))


def _read(path):
    return torch.frombuffer(bytearray(open(path, "rb").read()),
                            dtype=torch.uint8)


def _check_loaded(dev_pages, shape, dtype=torch.bfloat16):
    """Loaded blocks equal the oracle's dequantized values bit for bit,
    every group is within 0.17 of its own amax, the rest stayed zero."""
    bb, gs, nl, nb = shape
    pages, ids, _, deq = cpu_pages(shape, dtype)
    others = [i for i in range(2 * nb + 2) if i not in set(ids)]
    for dev, page, y in zip(dev_pages, pages, deq):
        got = dev.cpu()
        assert_bits(got[ids], y, "loaded pages")
        assert_group_bound(got[ids], page[ids], gs)
        assert (got[others].view(torch.int16) == 0).all()


def _engine_roundtrip(tmp_path, shape, copy_path, dtype=torch.bfloat16, **kw):
    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape, dtype)
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(dev_pages, tmp_path, shape, copy_path,
                                       **kw)
    store.transfer_async([0x71], {0: ids})
    assert wait_finished(store)[0].success
    data = _read(mapper.file_name(0x71, 0))
    for t in dev_pages:
        t.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0x71], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    _check_loaded(dev_pages, shape, dtype)
    return eng, data, want


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_gpu_engine_roundtrip_matches_oracle(tmp_path, shape, copy_path):
    bb, gs, nl, nb = shape
    _, data, want = _engine_roundtrip(tmp_path, shape, copy_path)
    assert data.numel() == nb * nl * record_bytes(bb, gs)
    assert_bytes(data, want, "file")


def _copier_roundtrip(shape, dtype=torch.bfloat16):
    from llm_d_kv_cache_amd.ops import block_copier

    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape, dtype)
    dev_pages = [p.cuda() for p in pages]
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
    for t in dev_pages:
        t.zero_()
    copier.scatter_fp4_group(0, ids, slab.data_ptr(), gs, stream)
    torch.cuda.synchronize()
    _check_loaded(dev_pages, shape, dtype)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] <= 128],
                         ids=_sid)
def test_gpu_block_copier_matches_oracle(shape):
    """BlockCopier.gather_fp4_group / scatter_fp4_group on device."""
    _copier_roundtrip(shape)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_gpu_scatter_of_every_code_byte(dt):
    """A hand-built slab holding all 256 code bytes under a spread of
    scales (every fp16 tie amax's among them), against the oracle decode."""
    from llm_d_kv_cache_amd.ops import block_copier

    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[dt]
    scales = decode_scales(dtype)
    slab, codes, scale = all_codes_slab(scales)
    tiles = scales.numel()
    page = torch.zeros(tiles + 1, 512, dtype=dtype, device="cuda")
    copier = block_copier([[page]])
    dev = slab.cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for lo in range(0, tiles, 128):
        ids = list(range(lo, min(lo + 128, tiles)))
        copier.scatter_fp4_group(0, ids, dev.data_ptr() + lo * 384, 16, stream)
    torch.cuda.synchronize()
    got = page.cpu()
    want = decode(codes.reshape(tiles, 32, 16), scale[..., None], dtype)
    assert_bits(got[:tiles], want.reshape(tiles, 512), "decoded slab")
    assert (got[tiles].view(torch.int16) == 0).all()


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_gpu_every_finite_input(dt):
    """Every finite bit pattern of the page type as x, each under several
    group amax values (fp4_group_oracle.exhaustive_groups, the input of the
    host-mode exhaustive test), through the device gather and scatter."""
    from llm_d_kv_cache_amd.ops import block_copier

    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[dt]
    x16 = exhaustive_groups(dtype)[0]
    bb, n = 8192, 4096
    blocks = -(-x16.numel() // n)
    page = torch.zeros(blocks, n, dtype=dtype)
    page.view(-1)[:x16.numel()] = x16.reshape(-1)
    ids = list(range(blocks))
    want = oracle_records([page], ids, 16)
    y = oracle(page, 16)[2]
    dev_page = page.cuda()
    copier = block_copier([[dev_page]])
    rec = record_bytes(bb, 16)
    slab = torch.zeros(blocks * rec, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for lo in range(0, blocks, 128):
        copier.gather_fp4_group(0, ids[lo:lo + 128],
                                slab.data_ptr() + lo * rec, 16, stream)
    torch.cuda.synchronize()
    assert_bytes(slab.cpu(), want, "slab")
    dev_page.zero_()
    for lo in range(0, blocks, 128):
        copier.scatter_fp4_group(0, ids[lo:lo + 128],
                                 slab.data_ptr() + lo * rec, 16, stream)
    torch.cuda.synchronize()
    assert_bits(dev_page.cpu(), y, "round trip")


@pytest.mark.parametrize("shape", FP16_SHAPES, ids=_sid)
def test_gpu_fp16_pages(tmp_path, shape):
    """fp16 pages: BlockCopier on device, then a staged engine round trip."""
    bb, gs, nl, nb = shape
    _copier_roundtrip(shape, torch.float16)
    eng, data, want = _engine_roundtrip(tmp_path, shape, "staged",
                                        torch.float16)
    assert eng.kv_dtype == "float16"
    assert_bytes(data, want, "file")


def _tie_pages():
    """(4, 11264) fp16 pages whose block 1 is the tie page: one G=16 group
    per fp16 amax at which two roundings and one differ on load."""
    page = make_pages(4, TIE_TILE_BYTES, 16, 1, seed=5, dtype=torch.float16)[0]
    page[1] = make_tie_page()[0]
    return [page]


def test_gpu_fp16_tie_page_scatter():
    """The load must round the f32 product, then round to fp16: a fused
    product-and-cast differs from the oracle in 682 elements of this page
    (asserted on the CPU in test_fp4_group.py)."""
    from llm_d_kv_cache_amd.ops import block_copier

    pages = _tie_pages()
    ids = [0, 1, 2, 3]
    want = oracle_records(pages, ids, 16)
    y = oracle(pages[0], 16)[2]
    dev_pages = [p.cuda() for p in pages]
    copier = block_copier([dev_pages])
    slab = torch.zeros(want.numel(), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    copier.gather_fp4_group(0, ids, slab.data_ptr(), 16, stream)
    torch.cuda.synchronize()
    assert_bytes(slab.cpu(), want, "slab")
    dev_pages[0].zero_()
    copier.scatter_fp4_group(0, ids, slab.data_ptr(), 16, stream)
    torch.cuda.synchronize()
    assert_bits(dev_pages[0].cpu(), y, "tie page through scatter_fp4_group")


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
def test_gpu_fp16_tie_page_engine(tmp_path, copy_path):
    pages = _tie_pages()
    ids = [0, 1, 2, 3]
    y = oracle(pages[0], 16)[2]
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(
        dev_pages, tmp_path, (TIE_TILE_BYTES, 16, 1, 4), copy_path)
    assert eng.kv_dtype == "float16"
    store.transfer_async([0x7E], {0: ids})
    assert wait_finished(store)[0].success
    assert_bytes(_read(mapper.file_name(0x7E, 0)),
                 oracle_records(pages, ids, 16), "file")
    dev_pages[0].zero_()
    torch.cuda.synchronize()
    load.transfer_async([0x7E], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    assert_bits(dev_pages[0].cpu(), y, "tie page through the engine")


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
def test_gpu_checksum_composes(tmp_path, copy_path):
    """checksum=True: payloads are the oracle's bytes, every footer
    verifies, the load passes verification and restores the pages."""
    from llm_d_kv_cache_amd.ops import block_copier

    shape = (8448, 128, 2, 4)
    bb, gs, nl, nb = shape
    eng, data, want = _engine_roundtrip(tmp_path, shape, copy_path,
                                        checksum=True)
    payload = record_bytes(bb, gs)
    tiles = nb * nl
    assert eng.group_geometry[0]["record_bytes"] == payload + 16
    assert data.numel() == tiles * (payload + 16)
    assert_bytes(data.reshape(tiles, payload + 16)[:, :payload].reshape(-1),
                 want, "payloads")
    host_copier = block_copier([[torch.zeros(1, bb // 2,
                                             dtype=torch.bfloat16)]])
    assert host_copier.verify_records(data.data_ptr(), tiles, payload) == \
        (0, -1)
    st = eng.stats()
    assert st.checksum_failures == 0 and st.errors == 0


def test_gpu_partial_load_with_skip(tmp_path):
    """24 blocks at 16 per file, then blocks 20-23 with
    skip_leading_blocks=20: the tail seek runs on fp4 record sizes."""
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
        assert_bits(got[20:24], oracle(page[20:24], gs)[2], "tail blocks")
        assert (got[:20].view(torch.int16) == 0).all()
        assert (got[24:].view(torch.int16) == 0).all()


def test_gpu_dram_tier_hit_after_file_deleted(tmp_path):
    """Staged path + pinned DRAM tier: the load is served from the resident
    fp4 slab (file deleted to prove it) and dequantized on device."""
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
    assert_bytes(resident, want, "DRAM slab")
    os.unlink(mapper.file_name(0xCA, 0))
    for t in dev_pages:
        t.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0xCA], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    assert eng.stats().host_cache_hits == 1
    _check_loaded(dev_pages, shape)
