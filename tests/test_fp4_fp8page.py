"""serialize="fp4_e2m1_group" over fp8 pages (kv_dtype="float8_e4m3fn") on
the host path.

An fp8 KV cache stores one OCP e4m3fn byte per element, so a tile of
block_bytes holds block_bytes elements and an fp4 record is block_bytes/2 +
4*block_bytes/G bytes. The host-mode codec must write exactly the bytes of
the torch oracle in fp4_fp8page_oracle.py (the HIP kernels are held to the
same bytes in test_fp4_fp8page_gpu.py), load back the oracle's page bytes,
0x80 for -0.0 and negative underflow included, and keep every group within
REL_BOUND (0.2, the exhaustive maximum the oracle recomputes) of its amax.

The input space is small enough to be covered whole: the exhaustive page
runs every finite x under every amax >= |x|, and a hand-built slab holds all
256 code bytes under each of the 126 scales an encoder can write.
"""
import os
import time

import pytest
import torch

from fp4_fp8page_oracle import (
    EXACT_CODES,
    EXACT_SCALE,
    EXHAUSTIVE_TILE_BYTES,
    GROUP_SIZES,
    REL_BOUND,
    all_codes_slab,
    as_u8,
    assert_bytes,
    assert_group_bound,
    assert_page_bits,
    decode,
    decode_scales,
    exhaustive_page,
    group_kind,
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
    tile_record_bytes,
)

F8 = torch.float8_e4m3fn
NUM_BLOCKS = 32
NUM_LAYERS = 2
BPF = 8

# (block_bytes, group_size): every group size at 2048, the smallest tiles
# (one and two groups per tile, 20- and 24-byte records) and a tile that is
# no multiple of 1 KiB
CASES = [(2048, g) for g in GROUP_SIZES] + [(32, 32), (32, 16), (1152, 128)]


def _engine(pages, tmp, model, gs, bpf=BPF, **kw):
    eng = TorchOffloadEngine(
        [pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=bpf,
                            copy_path="host", serialize="fp4_e2m1_group",
                            fp4_group_size=gs, **kw))
    tag = f"{eng.kv_dtype}+fp4g{gs}" + ("+ck" if kw.get("checksum") else "")
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(model=model, dtype=tag))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [bpf]),
            StorageToGPUHandler(eng, mapper, [bpf]))


def _read(path):
    return torch.frombuffer(bytearray(open(path, "rb").read()),
                            dtype=torch.uint8)


def _zero(pages):
    for p in pages:
        as_u8(p).zero_()


@pytest.fixture(scope="module", params=CASES,
                ids=[f"bb{b}-g{g}" for b, g in CASES])
def roundtrip(request, tmp_path_factory):
    """One host-mode store + load per case, shared by the checks below."""
    bb, gs = request.param
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=bb + gs)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(
        pages, tmp_path_factory.mktemp("fp4f8"), "fp4f8", gs)
    ids = list(range(1, 2 * BPF, 2))  # 8 odd blocks -> one file
    store.transfer_async([0x41], {0: ids})
    assert wait_finished(store)[0].success
    data = _read(mapper.file_name(0x41, 0))
    _zero(pages)
    load.transfer_async([0x41], {0: ids})
    assert wait_finished(load)[0].success
    return dict(bb=bb, gs=gs, ids=ids, orig=orig, pages=pages, data=data,
                eng=eng)


def test_rel_bound_is_the_exhaustive_maximum():
    assert 0.19 < REL_BOUND <= 0.2 + 1e-6


def test_record_bytes_in_geometry(roundtrip):
    r = roundtrip
    bb, gs = r["bb"], r["gs"]
    assert record_bytes(bb, gs) == bb // 2 + 4 * bb // gs
    assert r["eng"].kv_dtype == "float8_e4m3fn"  # auto, from the tensors
    assert r["eng"].group_geometry[0]["record_bytes"] == record_bytes(bb, gs)
    assert tile_record_bytes("fp4_e2m1_group", bb, 128, fp4_group_size=gs,
                             kv_dtype="float8_e4m3fn") == record_bytes(bb, gs)
    assert tile_record_bytes("fp4_e2m1_group", bb, 128, checksum=True,
                             fp4_group_size=gs, kv_dtype="float8_e4m3fn") == \
        record_bytes(bb, gs) + 16
    assert tile_record_bytes("raw", bb, 128, kv_dtype="float8_e4m3fn") == bb


def test_bits_per_element():
    """4 + 32/G bits per element: 5 at G=32, 1.6x below the fp8 page; and
    the 16-bit default of tile_record_bytes is unchanged."""
    for g, bits in ((16, 6.0), (32, 5.0), (64, 4.5), (128, 4.25)):
        assert record_bytes(4096, g) * 8 == bits * 4096
    assert tile_record_bytes("fp4_e2m1_group", 4096, 128,
                             fp4_group_size=32) == 1024 + 256
    assert record_bytes(32, 32) == 20 and record_bytes(32, 16) == 24


def test_file_bytes_equal_oracle(roundtrip):
    r = roundtrip
    assert r["data"].numel() == \
        BPF * NUM_LAYERS * record_bytes(r["bb"], r["gs"])
    assert_bytes(r["data"], oracle_records(r["orig"], r["ids"], r["gs"]),
                 "file")


def test_loaded_pages_equal_oracle(roundtrip):
    r = roundtrip
    untouched = [i for i in range(NUM_BLOCKS) if i not in r["ids"]]
    saw_negative_zero = False
    for page, o in zip(r["pages"], r["orig"]):
        y = oracle(o[r["ids"]], r["gs"])[2]
        assert_page_bits(page[r["ids"]], y, "loaded pages")
        assert (as_u8(page)[untouched] == 0).all()
        saw_negative_zero |= bool((y == 0x80).any())
    assert saw_negative_zero  # the inputs do reach the 0x80 path


def test_per_group_accuracy(roundtrip):
    r = roundtrip
    for page, o in zip(r["pages"], r["orig"]):
        assert_group_bound(page[r["ids"]], o[r["ids"]], r["gs"])


def test_planted_groups(roundtrip):
    """The exact group's first 16 elements sit on every e2m1 value and tie,
    their codes are fixed by the format and -0.0 / -2^-9 load as 0x80; an
    all-zero group stores scale 1/6 and returns zeros."""
    r = roundtrip
    bb, gs = r["bb"], r["gs"]
    ng = bb // gs
    rec = record_bytes(bb, gs)
    want = torch.tensor(EXACT_CODES, dtype=torch.uint8)
    want = want[0::2] | (want[1::2] << 4)
    six = torch.full((1,), 6.0)
    one_sixth = torch.div(torch.ones(1), six)
    sub_scale = torch.div(torch.full((1,), 7 * 2.0 ** -9), six)
    kinds = set()
    for li, page in enumerate(r["pages"]):
        for bi, b in enumerate(r["ids"]):
            record = r["data"][(bi * NUM_LAYERS + li) * rec:][:rec]
            scales = record[bb // 2:].view(torch.float32)
            for j in range(ng):
                kind = group_kind(b, j, ng)
                kinds.add(kind)
                got = as_u8(page)[b, j * gs:(j + 1) * gs]
                if kind == "exact":
                    assert torch.equal(record[j * gs // 2:][:8], want)
                    assert scales[j].item() == EXACT_SCALE
                    assert got[13] == 0x80 and got[14] == 0x80
                elif kind == "zero":
                    assert scales[j].item() == one_sixth.item()
                    assert (record[j * gs // 2:][:gs // 2] == 0).all()
                    assert (got == 0).all()
                elif kind == "sub":
                    assert scales[j].item() == sub_scale.item()
    assert kinds == {"zero", "sub", "exact", "random"}


# ---- the whole input space through the host codec ----------------------------

def _copier_roundtrip(page, gs):
    """uint8 (blocks, bb) -> host BlockCopier gather + scatter. Returns (the
    packed records, the loaded page bytes)."""
    from llm_d_kv_cache_amd.ops import block_copier

    blocks, bb = page.shape
    work = page.clone().view(F8)
    copier = block_copier([[work]])
    rec = record_bytes(bb, gs)
    assert copier.packed_bytes_fp4_group(0, 1, gs) == rec
    slab = torch.zeros(blocks * rec, dtype=torch.uint8)
    ids = list(range(blocks))
    copier.gather_fp4_group(0, ids, slab.data_ptr(), gs, 0)
    as_u8(work).zero_()
    copier.scatter_fp4_group(0, ids, slab.data_ptr(), gs, 0)
    return slab, as_u8(work)


def test_exhaustive_page():
    """Every finite x under every amax >= |x|, G=16 groups [amax, 15 x]."""
    page = exhaustive_page()
    assert page.shape[1] == EXHAUSTIVE_TILE_BYTES and page.shape[0] <= 128
    slab, loaded = _copier_roundtrip(page, 16)
    assert_bytes(slab, oracle_records([page], list(range(page.shape[0])), 16),
                 "host codec records")
    assert_page_bits(loaded, oracle(page, 16)[2], "host codec round trip")
    assert_group_bound(loaded, page, 16)


def test_every_code_byte_under_every_scale():
    """A hand-built slab: all 256 code bytes under each of the 126 scales
    amax/6, through the host scatter."""
    from llm_d_kv_cache_amd.ops import block_copier

    scales = decode_scales()
    assert scales.numel() == 126
    slab, codes, scale = all_codes_slab(scales)
    tiles = scales.numel()
    page = torch.zeros(tiles, 512, dtype=torch.uint8).view(F8)
    copier = block_copier([[page]])
    assert copier.packed_bytes_fp4_group(0, 1, 16) == 384
    copier.scatter_fp4_group(0, list(range(tiles)), slab.data_ptr(), 16, 0)
    want = decode(codes.reshape(tiles, 32, 16), scale[..., None])
    assert_page_bits(page, want.reshape(tiles, 512), "decoded slab")
    # -0.0 comes back as 0x80: code 0x8 is the high nibble of byte 0x80
    assert (as_u8(page)[:, 2 * 0x80 + 1] == 0x80).all()
    assert ((want & 0x7f) != 0x7f).all()  # no load reaches the NaN code


@pytest.mark.parametrize("gs", GROUP_SIZES)
def test_block_copier_slab_with_checksum_stride(gs):
    """BlockCopier slabs equal the oracle, dense and with the footer
    stride; the footers seal and verify."""
    from llm_d_kv_cache_amd.ops import block_copier

    bb = 1152 if gs == 128 else 2048
    pages = make_pages(6, bb, gs, NUM_LAYERS, seed=gs)
    orig = [p.clone() for p in pages]
    ids = [5, 0, 3]
    want = oracle_records(orig, ids, gs)
    copier = block_copier([pages])
    payload = record_bytes(bb, gs)
    tiles = len(ids) * NUM_LAYERS
    slab = torch.zeros(copier.packed_bytes_fp4_group(0, len(ids), gs),
                       dtype=torch.uint8)
    assert slab.numel() == tiles * payload
    copier.gather_fp4_group(0, ids, slab.data_ptr(), gs, 0)
    assert_bytes(slab, want, "slab")
    sealed = torch.zeros(
        copier.packed_bytes_fp4_group(0, len(ids), gs, checksum=True),
        dtype=torch.uint8)
    assert sealed.numel() == tiles * (payload + 16)
    copier.gather_fp4_group(0, ids, sealed.data_ptr(), gs, 0, checksum=True)
    copier.seal_records(sealed.data_ptr(), tiles, payload, 0)
    assert copier.verify_records(sealed.data_ptr(), tiles, payload, 0) == \
        (0, -1)
    assert_bytes(sealed.reshape(tiles, payload + 16)[:, :payload].reshape(-1),
                 want, "payloads")
    _zero(pages)
    copier.scatter_fp4_group(0, ids, sealed.data_ptr(), gs, 0, checksum=True)
    for page, o in zip(pages, orig):
        assert_page_bits(page[ids], oracle(o[ids], gs)[2], "scattered")


# ---- composition with the rest of the engine --------------------------------

def test_checksum_composes(tmp_path):
    """checksum=True: footers verify, and a flipped code bit fails the load
    and leaves the pages untouched."""
    from llm_d_kv_cache_amd.ops import block_copier

    bb, gs = 2048, 32
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=17)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(pages, tmp_path, "fp4f8-ck", gs,
                                       checksum=True)
    payload = record_bytes(bb, gs)
    assert eng.group_geometry[0]["record_bytes"] == payload + 16
    ids = list(range(BPF))
    store.transfer_async([0xC4], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0xC4, 0)
    data = _read(path)
    tiles = BPF * NUM_LAYERS
    assert data.numel() == tiles * (payload + 16)
    assert_bytes(data.reshape(tiles, payload + 16)[:, :payload].reshape(-1),
                 oracle_records(orig, ids, gs), "payloads")
    copier = block_copier([pages])
    assert copier.verify_records(data.data_ptr(), tiles, payload, 0) == (0, -1)
    assert copier.packed_bytes_fp4_group(0, BPF, gs, checksum=True) == \
        data.numel()
    _zero(pages)
    load.transfer_async([0xC4], {0: ids})
    assert wait_finished(load)[0].success
    for page, o in zip(pages, orig):
        assert_page_bits(page[ids], oracle(o[ids], gs)[2], "loaded pages")
    # one flipped code bit in record 5
    data[5 * (payload + 16) + 33] ^= 0x10
    with open(path, "wb") as f:
        f.write(data.numpy().tobytes())
    for p in pages:
        as_u8(p).fill_(0x38)  # 1.0
    load.transfer_async([0xC4], {0: ids})
    assert not wait_finished(load)[0].success
    assert eng.stats().checksum_failures == 1
    for p in pages:
        assert (as_u8(p) == 0x38).all()


def test_partial_and_offset_loads(tmp_path):
    """24 blocks at 16 per file; blocks 20-23 are tail-seeked out of the
    second (short) file by record size."""
    bb, gs, bpf = 2048, 32, 16
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=7)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(pages, tmp_path, "fp4f8-part", gs,
                                       bpf=bpf)
    store.transfer_async([0xB1, 0xB2], {0: list(range(24))})
    assert wait_finished(store)[0].success
    rec = record_bytes(bb, gs)
    assert os.path.getsize(mapper.file_name(0xB1, 0)) == 16 * NUM_LAYERS * rec
    assert os.path.getsize(mapper.file_name(0xB2, 0)) == 8 * NUM_LAYERS * rec
    _zero(pages)
    load.transfer_async([0xB1, 0xB2], {0: list(range(20, 24))},
                        skip_leading_blocks=20)
    assert wait_finished(load)[0].success
    for page, o in zip(pages, orig):
        assert_page_bits(page[20:24], oracle(o[20:24], gs)[2], "tail blocks")
        assert (as_u8(page)[:20] == 0).all()
        assert (as_u8(page)[24:] == 0).all()


def test_dram_cache_and_writeback(tmp_path):
    """Composed with the pinned cache + write-back: the flush writes the fp4
    file, and a DRAM hit serves after the file is deleted."""
    bb, gs = 2048, 64
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=11)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(
        pages, tmp_path, "fp4f8-wb", gs, host_cache_bytes=64 << 20,
        write_policy="back")
    ids = list(range(BPF))
    store.transfer_async([0xFB], {0: ids})
    assert wait_finished(store)[0].success
    deadline = time.time() + 10
    while eng.stats().writeback_flushes < 1 and time.time() < deadline:
        time.sleep(0.005)
    path = mapper.file_name(0xFB, 0)
    assert_bytes(_read(path), oracle_records(orig, ids, gs), "flushed file")
    os.unlink(path)
    _zero(pages)
    load.transfer_async([0xFB], {0: ids})
    assert wait_finished(load)[0].success
    assert eng.stats().host_cache_hits >= 1
    for page, o in zip(pages, orig):
        assert_page_bits(page[ids], oracle(o[ids], gs)[2], "DRAM-tier load")


def test_obj_tier_roundtrip():
    """ObjStorageEngine over fp8 pages against the in-repo fake S3: the
    object holds the oracle's bytes, a ranged partial load lands, and the
    fp8 modes are refused."""
    import threading

    from test_obj_backend import ThreadingHTTPServer, _FakeS3

    from llm_d_kv_cache_amd.offload.obj_backend import (
        ObjKeyMapper, ObjStorageConfig, ObjStorageEngine)

    bb, gs = 2048, 32
    _FakeS3.store = {}
    srv = ThreadingHTTPServer(("127.0.0.1", 0), _FakeS3)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        pages = make_pages(16, bb, gs, NUM_LAYERS, seed=6)
        orig = [p.clone() for p in pages]
        eng = ObjStorageEngine(
            [pages],
            ObjStorageConfig(endpoint=f"http://127.0.0.1:{srv.server_port}",
                             serialize="fp4_e2m1_group", fp4_group_size=gs))
        assert eng.kv_dtype == "float8_e4m3fn"
        assert eng.group_geometry[0]["record_bytes"] == record_bytes(bb, gs)
        mapper = ObjKeyMapper(FileMapper("/kv", KVCacheLayoutConfig(
            model="objf8", dtype="float8_e4m3fn+fp4g32")))
        store = GPUToStorageHandler(eng, mapper, [8])
        load = StorageToGPUHandler(eng, mapper, [8])
        ids = list(range(8))
        store.transfer_async([0xE4], {0: ids})
        assert wait_finished(store)[0].success
        (obj,) = _FakeS3.store.values()
        assert_bytes(torch.frombuffer(bytearray(obj), dtype=torch.uint8),
                     oracle_records(orig, ids, gs), "object")
        _zero(pages)
        load.transfer_async([0xE4], {0: [6, 7]}, skip_leading_blocks=6)
        assert wait_finished(load)[0].success
        for page, o in zip(pages, orig):
            assert_page_bits(page[6:8], oracle(o[6:8], gs)[2], "ranged load")
            assert (as_u8(page)[:6] == 0).all()
        eng.close()
        for mode in ("fp8_e4m3", "fp8_e4m3_group"):
            with pytest.raises(ValueError, match="raw.*fp4_e2m1_group"):
                ObjStorageEngine([pages], ObjStorageConfig(serialize=mode))
    finally:
        srv.shutdown()


def test_raw_over_fp8_pages(tmp_path):
    """serialize="raw" takes the format trivially: the file is the pages."""
    pages = make_pages(NUM_BLOCKS, 2048, 32, NUM_LAYERS, seed=3)
    orig = [p.clone() for p in pages]
    eng = TorchOffloadEngine(
        [pages], OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=BPF,
                                     copy_path="host",
                                     kv_dtype="float8_e4m3fn"))
    assert eng.kv_dtype == "float8_e4m3fn"
    mapper = FileMapper(str(tmp_path), KVCacheLayoutConfig(
        model="raw-f8", dtype="float8_e4m3fn"))
    store = GPUToStorageHandler(eng, mapper, [BPF])
    ids = list(range(BPF))
    store.transfer_async([0x52], {0: ids})
    assert wait_finished(store)[0].success
    want = torch.stack([as_u8(o)[ids] for o in orig], dim=1).reshape(-1)
    assert_bytes(_read(mapper.file_name(0x52, 0)), want, "raw file")


# ---- resolution and errors ----------------------------------------------------

def _fp4(**kw):
    return OffloadEngineConfig(copy_path="host", serialize="fp4_e2m1_group",
                               io_threads=1, **kw)


def test_auto_resolution(tmp_path):
    """float8_e4m3fn tensors resolve to the fp8 page format; uint8 views
    keep resolving to bfloat16 and need the explicit value, which then gives
    the same bytes as the typed tensors."""
    from llm_d_kv_cache_amd.offload.engine import KV_DTYPES, resolve_kv_dtype
    from llm_d_kv_cache_amd.ops import block_copier

    assert KV_DTYPES == ("bfloat16", "float16", "float8_e4m3fn")
    bb, gs = 2048, 32
    f8 = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=5)
    views = [as_u8(p.clone()) for p in f8]
    assert resolve_kv_dtype([f8], "auto") == "float8_e4m3fn"
    assert resolve_kv_dtype([f8], "float8_e4m3fn") == "float8_e4m3fn"
    assert resolve_kv_dtype([views], "auto") == "bfloat16"
    assert resolve_kv_dtype([views], "float8_e4m3fn") == "float8_e4m3fn"
    assert resolve_kv_dtype([f8, views], "auto") == "bfloat16"
    assert resolve_kv_dtype([f8, views], "float8_e4m3fn") == "float8_e4m3fn"
    assert TorchOffloadEngine([f8], _fp4()).kv_dtype == "float8_e4m3fn"
    auto_views = TorchOffloadEngine([views], _fp4())
    assert auto_views.kv_dtype == "bfloat16"
    assert auto_views.group_geometry[0]["record_bytes"] == \
        bb // 4 + 4 * (bb // 2) // gs
    # explicit value on opaque views: store and load, the oracle's bytes
    eng, mapper, store, load = _engine(views, tmp_path, "u8-f8", gs,
                                       kv_dtype="float8_e4m3fn")
    assert eng.kv_dtype == "float8_e4m3fn"
    ids = list(range(BPF))
    store.transfer_async([0x34], {0: ids})
    assert wait_finished(store)[0].success
    assert_bytes(_read(mapper.file_name(0x34, 0)),
                 oracle_records(f8, ids, gs), "uint8-view file")
    _zero(views)
    load.transfer_async([0x34], {0: ids})
    assert wait_finished(load)[0].success
    for v, o in zip(views, f8):
        assert_page_bits(v[ids], oracle(o[ids], gs)[2], "uint8-view load")
    # the copier resolves the same way
    assert block_copier([f8]).packed_bytes_fp4_group(0, 1, gs) == \
        NUM_LAYERS * record_bytes(bb, gs)
    assert block_copier([views]).packed_bytes_fp4_group(0, 1, gs) == \
        NUM_LAYERS * (bb // 4 + 4 * (bb // 2) // gs)
    assert block_copier([views], kv_dtype="float8_e4m3fn") \
        .packed_bytes_fp4_group(0, 1, gs) == NUM_LAYERS * record_bytes(bb, gs)


def test_config_errors():
    from llm_d_kv_cache_amd import ensure_offload_native
    from llm_d_kv_cache_amd.ops import block_copier

    f8 = [torch.zeros(4, 2048, dtype=torch.uint8).view(F8)]
    bf = [torch.zeros(4, 1024, dtype=torch.bfloat16)]
    f16 = [torch.zeros(4, 1024, dtype=torch.float16)]
    u8 = [torch.zeros(4, 2048, dtype=torch.uint8)]

    # the fp8 modes do not apply to fp8 pages, typed or declared
    for mode in ("fp8_e4m3", "fp8_e4m3_group"):
        def cfg(**kw):
            return OffloadEngineConfig(copy_path="host", serialize=mode, **kw)
        with pytest.raises(ValueError, match="raw.*fp4_e2m1_group"):
            TorchOffloadEngine([f8], cfg())
        with pytest.raises(ValueError, match="raw.*fp4_e2m1_group"):
            TorchOffloadEngine([u8], cfg(kv_dtype="float8_e4m3fn"))
        with pytest.raises(ValueError, match="raw.*fp4_e2m1_group"):
            tile_record_bytes(mode, 2048, 128, kv_dtype="float8_e4m3fn")
    # an explicit value against the tensors' own dtype, both directions
    with pytest.raises(ValueError, match="kv_dtype.*bfloat16.*float8_e4m3fn"):
        TorchOffloadEngine([f8], _fp4(kv_dtype="bfloat16"))
    with pytest.raises(ValueError, match="kv_dtype.*float16.*float8_e4m3fn"):
        TorchOffloadEngine([f8], _fp4(kv_dtype="float16"))
    with pytest.raises(ValueError, match="kv_dtype.*float8_e4m3fn.*bfloat16"):
        TorchOffloadEngine([bf], _fp4(kv_dtype="float8_e4m3fn"))
    with pytest.raises(ValueError, match="kv_dtype.*float8_e4m3fn.*float16"):
        TorchOffloadEngine([f16], _fp4(kv_dtype="float8_e4m3fn"))
    # float8 next to 16-bit tensors, in one group or across groups
    with pytest.raises(ValueError, match="mix"):
        TorchOffloadEngine([f8, bf], _fp4())
    with pytest.raises(ValueError, match="mix"):
        TorchOffloadEngine([f8, f16], _fp4(kv_dtype="float8_e4m3fn"))
    # the other fp8 formats are no page format of any converting mode
    for dt in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        other = [torch.zeros(4, 2048, dtype=torch.uint8).view(dt)]
        for mode in ("fp8_e4m3", "fp8_e4m3_group", "fp4_e2m1_group"):
            with pytest.raises(ValueError, match="float8_e4m3fn"):
                TorchOffloadEngine([other], OffloadEngineConfig(
                    copy_path="host", serialize=mode))
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            TorchOffloadEngine([other], _fp4(kv_dtype="float8_e4m3fn"))
        TorchOffloadEngine([other], OffloadEngineConfig(copy_path="host"))
    # spelling; the accepted values are listed, 16-bit ones first
    with pytest.raises(ValueError,
                       match="auto.*bfloat16.*float16.*float8_e4m3fn"):
        TorchOffloadEngine([f8], _fp4(kv_dtype="fp8"))
    with pytest.raises(ValueError, match="kv_dtype"):
        tile_record_bytes("raw", 2048, 128, kv_dtype="fp8")
    # G must divide block_bytes elements: 2064 = 129 * 16
    odd = [torch.zeros(4, 2064, dtype=torch.uint8).view(F8)]
    with pytest.raises(ValueError, match=r"group 0.*2064.*2064.*8-bit.*32"):
        TorchOffloadEngine([odd], _fp4())
    TorchOffloadEngine([odd], _fp4(fp4_group_size=16))
    with pytest.raises(ValueError, match="fp4_group_size.*48"):
        TorchOffloadEngine([f8], _fp4(fp4_group_size=48))

    # the bindings reject what the wrappers reject
    ko = ensure_offload_native()
    groups = [([f8[0].data_ptr()], [2048], 2048, 4)]
    for mode in ("fp8_e4m3", "fp8_e4m3_group"):
        with pytest.raises(ValueError, match="raw.*fp4_e2m1_group"):
            ko.StorageOffloadEngine(groups, io_threads=1, copy_path="host",
                                    serialize=mode, kv_dtype="float8_e4m3fn")
    with pytest.raises(ValueError, match="kv_dtype.*bfloat16.*float16"):
        ko.StorageOffloadEngine(groups, io_threads=1, copy_path="host",
                                kv_dtype="float8_e4m3fnuz")
    odd_groups = [([odd[0].data_ptr()], [2064], 2064, 4)]
    with pytest.raises(ValueError, match="group 0.*2064.*32"):
        ko.StorageOffloadEngine(odd_groups, io_threads=1, copy_path="host",
                                serialize="fp4_e2m1_group",
                                kv_dtype="float8_e4m3fn")
    ko.StorageOffloadEngine(groups, io_threads=1, copy_path="host",
                            kv_dtype="float8_e4m3fn")  # raw

    # a copier over fp8 pages has the raw and the fp4 methods only
    copier = block_copier([f8])
    slab = torch.zeros(1 << 16, dtype=torch.uint8)
    assert copier.packed_bytes(0, 2) == 2 * 2048
    assert copier.packed_bytes_fp4_group(0, 2, 128) == 2 * (1024 + 64)
    for call in (lambda: copier.packed_bytes_fp8(0, 1),
                 lambda: copier.packed_bytes_fp8_group(0, 1, 128),
                 lambda: copier.gather_fp8(0, [0], slab.data_ptr(), 0, 0),
                 lambda: copier.scatter_fp8(0, [0], slab.data_ptr(), 0),
                 lambda: copier.gather_fp8_group(0, [0], slab.data_ptr(),
                                                 128, 0),
                 lambda: copier.scatter_fp8_group(0, [0], slab.data_ptr(),
                                                  128, 0)):
        with pytest.raises(ValueError, match="already are fp8"):
            call()
    assert (slab == 0).all() and (as_u8(f8[0]) == 0).all()
    with pytest.raises(ValueError, match="group_size"):
        copier.packed_bytes_fp4_group(0, 1, 48)
    with pytest.raises(ValueError, match="not a multiple"):
        block_copier([odd]).gather_fp4_group(0, [0], slab.data_ptr(), 32, 0)
    with pytest.raises(ValueError, match="kv_dtype"):
        block_copier([bf], kv_dtype="float8_e4m3fn")


def _peer_guard_rank(rank, init_file, q):
    """Runs in a child process (a process group is per process): one rank
    of a two-rank gloo world over float8 pages."""
    try:
        import torch.distributed as dist

        from llm_d_kv_cache_amd.peer import PeerMigrationService

        dist.init_process_group("gloo", init_method=f"file://{init_file}",
                                rank=rank, world_size=2)
        ctrl_pg = dist.new_group(backend="gloo")
        data_pg = dist.new_group(backend="gloo")
        f8 = make_pages(4, 2048, 32, 1, seed=40 + rank)
        svc = PeerMigrationService([f8], data_group=data_pg,
                                   control_group=ctrl_pg)
        assert svc.kv_dtype == "float8_e4m3fn"
        for call in (
                lambda: svc.pull(0x1, 0, [0], src_rank=1, fp8=True),
                lambda: svc.pull_many([(0x1, 0, [0])], src_rank=1, fp8=True)):
            try:
                call()
            except ValueError as e:
                assert "raw" in str(e), e
            else:
                raise AssertionError("fp8 pull on float8 pages did not raise")
        if rank == 1:
            svc.register_blocks(0x1, 0, [1, 2])
        dist.barrier()
        if rank == 0:
            # a raw pull moves the peer's page bytes
            theirs = make_pages(4, 2048, 32, 1, seed=41)
            assert svc.pull(0x1, 0, [3, 0], src_rank=1).result(timeout=30)
            assert torch.equal(as_u8(f8[0])[[3, 0]], as_u8(theirs[0])[[1, 2]])
        dist.barrier()
        svc.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"FAIL: {e}\n{traceback.format_exc()}"))


def test_peer_service_guards(tmp_path):
    """A PeerMigrationService over float8 pages pulls raw; asking it for an
    fp8 pull raises before anything is queued."""
    import multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_peer_guard_rank,
                         args=(r, str(tmp_path / "pg_init"), q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
    assert all(v == "ok" for v in results.values()), results
