"""serialize="fp4_e2m1_group" on the host path: OCP e2m1 codes, two per
byte, one f32 scale per fp4_group_size elements.

The host-mode software codec must write exactly the bytes of the torch
oracle in fp4_group_oracle.py (the HIP kernels are held to the same bytes
in test_fp4_group_gpu.py), load back the oracle's values bit for bit, and
keep every group within 0.17 of its OWN amax (the derived bound: half the
widest e2m1 gap is amax/6).

The exhaustive tests place every finite bf16 / fp16 bit pattern as x in
G=16 groups. Patterns are sorted by magnitude and taken 15 at a time; each
run of 15 is stored once per amax in a list built from its own largest
magnitude m (m itself, and about 1.3 m, 2.7 m and 6.5 m, so t = x * inv
lands near 6, 4.5, 2.2 and 0.9) and from a fixed ladder that holds values
below and above 1 (every ladder entry >= m is used). A group's amax can
never be smaller than its x, so a pattern at the top of the format sees
fewer different amax values than one in the middle; the test asserts at
least four for every pattern whose magnitude leaves room for them.
"""
import logging
import os
import time

import pytest
import torch

from fp4_group_oracle import (
    EXACT_CODES,
    GROUP_SIZES,
    TIE_TILE_BYTES,
    all_codes_slab,
    assert_bits,
    assert_bytes,
    assert_group_bound,
    decode,
    decode_scales,
    exhaustive_groups,
    fp16_tie_amaxes,
    make_pages,
    make_tie_page,
    oracle,
    oracle_records,
    record_bytes,
    single_rounding_y,
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

NUM_BLOCKS = 32
NUM_LAYERS = 2
BPF = 8
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}

# (block_bytes, group_size, dtype): every group size and both page types at
# 4096, and a tile that is no multiple of 1 KiB (384 elements)
CASES = [(4096, g, d) for g in GROUP_SIZES for d in DTYPES] + \
    [(768, 32, "bf16"), (768, 128, "fp16")]


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


@pytest.fixture(scope="module", params=CASES,
                ids=[f"bb{b}-g{g}-{d}" for b, g, d in CASES])
def roundtrip(request, tmp_path_factory):
    """One host-mode store + load per case, shared by the checks below."""
    bb, gs, dt = request.param
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=bb + gs,
                       dtype=DTYPES[dt])
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(
        pages, tmp_path_factory.mktemp("fp4g"), "fp4g", gs)
    ids = list(range(1, 2 * BPF, 2))  # 8 odd blocks -> one file
    store.transfer_async([0x41], {0: ids})
    assert wait_finished(store)[0].success
    data = _read(mapper.file_name(0x41, 0))
    for p in pages:
        p.zero_()
    load.transfer_async([0x41], {0: ids})
    assert wait_finished(load)[0].success
    return dict(bb=bb, gs=gs, dt=dt, ids=ids, orig=orig, pages=pages,
                data=data, eng=eng)


def test_record_bytes_in_geometry(roundtrip):
    r = roundtrip
    n = r["bb"] // 2
    assert record_bytes(r["bb"], r["gs"]) == n // 2 + 4 * n // r["gs"]
    assert r["eng"].group_geometry[0]["record_bytes"] == \
        record_bytes(r["bb"], r["gs"])
    assert tile_record_bytes("fp4_e2m1_group", r["bb"], 128,
                             fp4_group_size=r["gs"]) == \
        record_bytes(r["bb"], r["gs"])
    assert r["eng"].kv_dtype == \
        {"bf16": "bfloat16", "fp16": "float16"}[r["dt"]]


def test_table_of_bytes_per_64_elements():
    for g, want in ((16, 48), (32, 40), (64, 36), (128, 34)):
        assert record_bytes(4096, g) * 64 == want * 2048
        assert tile_record_bytes("fp4_e2m1_group", 4096, 128,
                                 fp4_group_size=g) == record_bytes(4096, g)
        assert tile_record_bytes("fp4_e2m1_group", 4096, 128, checksum=True,
                                 fp4_group_size=g) == \
            record_bytes(4096, g) + 16


def test_file_bytes_equal_oracle(roundtrip):
    r = roundtrip
    assert r["data"].numel() == BPF * NUM_LAYERS * record_bytes(r["bb"], r["gs"])
    assert_bytes(r["data"], oracle_records(r["orig"], r["ids"], r["gs"]),
                 "file")


def test_loaded_values_equal_oracle(roundtrip):
    r = roundtrip
    untouched = [i for i in range(NUM_BLOCKS) if i not in r["ids"]]
    for page, o in zip(r["pages"], r["orig"]):
        _, _, y, _ = oracle(o[r["ids"]], r["gs"])
        assert_bits(page[r["ids"]], y, "loaded pages")
        assert (page[untouched].view(torch.int16) == 0).all()


def test_per_group_accuracy(roundtrip):
    r = roundtrip
    for page, o in zip(r["pages"], r["orig"]):
        assert_group_bound(page[r["ids"]], o[r["ids"]], r["gs"])


def test_planted_codes(roundtrip):
    """The exact group's first 16 elements sit on every e2m1 value and
    every tie; their codes are fixed by the format, and an all-zero group
    stores scale 1/6 and returns zeros."""
    r = roundtrip
    n = r["bb"] // 2
    ng = n // r["gs"]
    rec = record_bytes(r["bb"], r["gs"])
    want = torch.tensor(EXACT_CODES, dtype=torch.uint8)
    want = want[0::2] | (want[1::2] << 4)
    one_sixth = torch.div(torch.ones(1), torch.full((1,), 6.0))
    for li, page in enumerate(r["pages"]):
        for bi, b in enumerate(r["ids"]):
            record = r["data"][(bi * NUM_LAYERS + li) * rec:][:rec]
            e = (b + 1) % ng
            assert torch.equal(record[e * r["gs"] // 2:][:8], want)
            scales = record[n // 2:].view(torch.float32)
            assert scales[e].item() == 0.125
            z = b % ng
            assert scales[z].item() == one_sixth.item()
            assert (record[z * r["gs"] // 2:][:r["gs"] // 2] == 0).all()
            assert (page[b, z * r["gs"]:(z + 1) * r["gs"]]
                    .view(torch.int16) == 0).all()


# ---- exhaustive encode / decode through the host codec -----------------------

def _host_codec(x, gs=16, bb=8192):
    """x: (groups, gs) values -> host BlockCopier gather + scatter on pages
    of bb bytes. Returns (packed records as the oracle lays them out, the
    loaded values)."""
    from llm_d_kv_cache_amd.ops import block_copier

    n = bb // 2
    flat = x.reshape(-1)
    blocks = -(-flat.numel() // n)
    page = torch.zeros(blocks, n, dtype=x.dtype)
    page.view(-1)[:flat.numel()] = flat
    orig = page.clone()
    copier = block_copier([[page]])
    rec = record_bytes(bb, gs)
    slab = torch.zeros(blocks * rec, dtype=torch.uint8)
    for lo in range(0, blocks, 128):
        ids = list(range(lo, min(lo + 128, blocks)))
        copier.gather_fp4_group(0, ids, slab[lo * rec:].data_ptr(), gs, 0)
    page.zero_()
    for lo in range(0, blocks, 128):
        ids = list(range(lo, min(lo + 128, blocks)))
        copier.scatter_fp4_group(0, ids, slab[lo * rec:].data_ptr(), gs, 0)
    return orig, slab, page


@pytest.mark.parametrize("dt", list(DTYPES))
def test_exhaustive_encode(dt):
    dtype = DTYPES[dt]
    x16, top, seen = exhaustive_groups(dtype)
    # how many different amax values each run of 15 patterns met
    distinct = torch.tensor([row[~row.isnan()].unique().numel()
                             for row in seen])
    roomy = top <= torch.finfo(dtype).max / 8
    assert (distinct[roomy] >= 4).all()
    below = (seen < 1).any(1)
    above = (seen > 1).any(1)
    assert above[top <= 1792].all() and below[top <= 0.8125].all()

    assert x16.shape[1] == 16
    orig, slab, loaded = _host_codec(x16)
    assert_bytes(slab, oracle_records([orig], list(range(orig.shape[0])), 16),
                 "host codec records")
    # (no error bound here: it is derived for results in the page type's
    # normal range, and these groups reach down into its subnormals)
    assert_bits(loaded, oracle(orig, 16)[2], "host codec round trip")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_exhaustive_decode(dt):
    """All 256 code bytes under a spread of scales, every fp16 tie amax's
    scale among them, through the host scatter."""
    from llm_d_kv_cache_amd.ops import block_copier

    dtype = DTYPES[dt]
    scales = decode_scales(dtype)
    assert scales.numel() >= 684 + 40
    slab, codes, scale = all_codes_slab(scales)
    tiles = scales.numel()
    page = torch.zeros(tiles, 512, dtype=dtype)
    copier = block_copier([[page]])
    assert copier.packed_bytes_fp4_group(0, tiles and 1, 16) == 384
    for lo in range(0, tiles, 128):
        ids = list(range(lo, min(lo + 128, tiles)))
        copier.scatter_fp4_group(0, ids, slab[lo * 384:].data_ptr(), 16, 0)
    want = decode(codes.reshape(tiles, 32, 16), scale[..., None], dtype)
    assert_bits(page, want.reshape(tiles, 512), "decoded slab")
    # -0.0 comes back as -0.0: code 0x8 is the high nibble of byte 0x80
    assert (page[:, 2 * 0x80 + 1].view(torch.int16) == -32768).all()


def _tie_pages():
    """(4, 11264) fp16 pages whose block 1 is the tie page."""
    page = make_pages(4, TIE_TILE_BYTES, 16, 1, seed=5, dtype=torch.float16)[0]
    page[1] = make_tie_page()[0]
    return [page]


def _assert_tie_page_separates_the_roundings():
    """The oracle's two roundings and a fused single rounding must differ
    on the tie page, or the page would not catch a fused product-and-cast.
    682 elements were reachable when checked with numpy."""
    ties = fp16_tie_amaxes()
    assert ties[1.5].numel() == 342 and ties[3.0].numel() == 342
    assert torch.cat(list(ties.values())).unique().numel() == 684
    page = make_tie_page()
    assert page.shape == (1, TIE_TILE_BYTES // 2)
    y = oracle(page, 16)[2]
    single = single_rounding_y(page, 16)
    differ = (y.view(torch.int16) != single.view(torch.int16)).sum().item()
    print(f"two roundings differ from one in {differ} elements")
    assert differ >= 600


def test_fp16_tie_page_host_roundtrip(tmp_path):
    """First the page itself (does it tell one rounding from two?), then
    the host codec against the oracle on it: BlockCopier and engine."""
    from llm_d_kv_cache_amd.ops import block_copier

    _assert_tie_page_separates_the_roundings()
    pages = _tie_pages()
    orig = [p.clone() for p in pages]
    y = oracle(orig[0], 16)[2]
    # BlockCopier
    copier = block_copier([pages])
    rec = record_bytes(TIE_TILE_BYTES, 16)
    slab = torch.zeros(4 * rec, dtype=torch.uint8)
    copier.gather_fp4_group(0, [0, 1, 2, 3], slab.data_ptr(), 16, 0)
    assert_bytes(slab, oracle_records(orig, [0, 1, 2, 3], 16), "slab")
    pages[0].zero_()
    copier.scatter_fp4_group(0, [0, 1, 2, 3], slab.data_ptr(), 16, 0)
    assert_bits(pages[0], y, "copier round trip")
    # engine
    pages[0].copy_(orig[0])
    eng, mapper, store, load = _engine(pages, tmp_path, "fp4g-tie", 16, bpf=4)
    assert eng.kv_dtype == "float16"
    store.transfer_async([0x7E], {0: [0, 1, 2, 3]})
    assert wait_finished(store)[0].success
    assert_bytes(_read(mapper.file_name(0x7E, 0)),
                 oracle_records(orig, [0, 1, 2, 3], 16), "file")
    pages[0].zero_()
    load.transfer_async([0x7E], {0: [0, 1, 2, 3]})
    assert wait_finished(load)[0].success
    assert_bits(pages[0], y, "engine round trip")


# ---- composition with the rest of the engine --------------------------------

@pytest.mark.parametrize("dt", list(DTYPES))
def test_checksum_composes(tmp_path, dt):
    """checksum=True: footers verify, and a flipped payload bit fails the
    load and leaves the pages untouched."""
    from llm_d_kv_cache_amd.ops import block_copier

    bb, gs = 4096, 32
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=17,
                       dtype=DTYPES[dt])
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(pages, tmp_path, "fp4g-ck", gs,
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
    assert copier.verify_records(data.data_ptr(), tiles, payload) == (0, -1)
    assert copier.packed_bytes_fp4_group(0, BPF, gs, checksum=True) == \
        data.numel()
    for p in pages:
        p.zero_()
    load.transfer_async([0xC4], {0: ids})
    assert wait_finished(load)[0].success
    for page, o in zip(pages, orig):
        assert_bits(page[ids], oracle(o[ids], gs)[2], "loaded pages")
    # one flipped code bit in record 5
    data[5 * (payload + 16) + 33] ^= 0x10
    with open(path, "wb") as f:
        f.write(data.numpy().tobytes())
    for p in pages:
        p.fill_(1.0)
    load.transfer_async([0xC4], {0: ids})
    assert not wait_finished(load)[0].success
    assert eng.stats().checksum_failures == 1
    for p in pages:
        assert (p == 1.0).all()


def test_partial_and_offset_loads(tmp_path):
    """24 blocks at 16 per file; blocks 20-23 are tail-seeked out of the
    second (short) file by record size."""
    bb, gs, bpf = 4096, 32, 16
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=7)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(pages, tmp_path, "fp4g-part", gs,
                                       bpf=bpf)
    store.transfer_async([0xB1, 0xB2], {0: list(range(24))})
    assert wait_finished(store)[0].success
    rec = record_bytes(bb, gs)
    assert os.path.getsize(mapper.file_name(0xB1, 0)) == 16 * NUM_LAYERS * rec
    assert os.path.getsize(mapper.file_name(0xB2, 0)) == 8 * NUM_LAYERS * rec
    for p in pages:
        p.zero_()
    load.transfer_async([0xB1, 0xB2], {0: list(range(20, 24))},
                        skip_leading_blocks=20)
    assert wait_finished(load)[0].success
    for page, o in zip(pages, orig):
        assert_bits(page[20:24], oracle(o[20:24], gs)[2], "tail blocks")
        assert (page[:20].view(torch.int16) == 0).all()
        assert (page[24:].view(torch.int16) == 0).all()


def test_dram_cache_and_writeback(tmp_path):
    """Composed with the pinned cache + write-back: the flush writes the fp4
    file, and a DRAM hit serves after the file is deleted."""
    bb, gs = 4096, 64
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=11)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(
        pages, tmp_path, "fp4g-wb", gs, host_cache_bytes=64 << 20,
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
    for p in pages:
        p.zero_()
    load.transfer_async([0xFB], {0: ids})
    assert wait_finished(load)[0].success
    assert eng.stats().host_cache_hits >= 1
    for page, o in zip(pages, orig):
        assert_bits(page[ids], oracle(o[ids], gs)[2], "DRAM-tier load")


def test_obj_tier_roundtrip():
    """ObjStorageEngine with the fp4 codec against the in-repo fake S3: the
    object holds the oracle's bytes, a ranged partial load lands."""
    import threading

    from test_obj_backend import ThreadingHTTPServer, _FakeS3

    from llm_d_kv_cache_amd.offload.obj_backend import (
        ObjKeyMapper, ObjStorageConfig, ObjStorageEngine)

    bb, gs = 4096, 32
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
        assert eng.group_geometry[0]["record_bytes"] == record_bytes(bb, gs)
        mapper = ObjKeyMapper(FileMapper("/kv", KVCacheLayoutConfig(
            model="objf4", dtype="bfloat16+fp4g32")))
        store = GPUToStorageHandler(eng, mapper, [8])
        load = StorageToGPUHandler(eng, mapper, [8])
        ids = list(range(8))
        store.transfer_async([0xE4], {0: ids})
        assert wait_finished(store)[0].success
        (obj,) = _FakeS3.store.values()
        assert_bytes(torch.frombuffer(bytearray(obj), dtype=torch.uint8),
                     oracle_records(orig, ids, gs), "object")
        for p in pages:
            p.zero_()
        load.transfer_async([0xE4], {0: [6, 7]}, skip_leading_blocks=6)
        assert wait_finished(load)[0].success
        for page, o in zip(pages, orig):
            assert_bits(page[6:8], oracle(o[6:8], gs)[2], "ranged load")
            assert (page[:6].view(torch.int16) == 0).all()
        eng.close()
        with pytest.raises(ValueError, match="fp4_group_size"):
            ObjStorageEngine([pages], ObjStorageConfig(
                serialize="fp4_e2m1_group", fp4_group_size=100))
    finally:
        srv.shutdown()


def test_peer_dram_lookup_always_misses(tmp_path, caplog):
    """The peer wire has no fp4 format: a lookup built for an fp4 engine
    reports a miss for a chunk that IS resident in the DRAM tier, and says
    so once."""
    from llm_d_kv_cache_amd.peer.tiered import make_dram_lookup

    bb, gs = 4096, 32
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=13)
    eng, mapper, store, _ = _engine(pages, tmp_path, "fp4g-peer", gs,
                                    host_cache_bytes=64 << 20)
    store.transfer_async([0x42], {0: list(range(BPF))})
    assert wait_finished(store)[0].success
    resident = eng.dram_chunk(mapper.file_name(0x42, 0), BPF, 0)
    assert resident is not None
    assert resident.numel() == BPF * NUM_LAYERS * record_bytes(bb, gs)
    lookup = make_dram_lookup(eng, mapper)
    with caplog.at_level(logging.WARNING,
                         logger="llm_d_kv_cache_amd.peer.tiered"):
        assert lookup(0x42, 0, BPF) is None
        assert lookup(0x42, 0, BPF) is None
    assert len([r for r in caplog.records
                if "fp4_e2m1_group" in r.getMessage()]) == 1


def test_config_errors():
    from llm_d_kv_cache_amd import ensure_offload_native
    from llm_d_kv_cache_amd.offload.engine import (
        FP4_GROUP_SIZES, SERIALIZE_MODES)
    from llm_d_kv_cache_amd.ops import block_copier

    assert FP4_GROUP_SIZES == (16, 32, 64, 128)
    assert "fp4_e2m1_group" in SERIALIZE_MODES
    assert OffloadEngineConfig().fp4_group_size == 32

    def cfg(**kw):
        return OffloadEngineConfig(copy_path="host",
                                   serialize="fp4_e2m1_group", **kw)

    pages = [torch.zeros(4, 2048, dtype=torch.bfloat16)]
    with pytest.raises(ValueError, match="fp4_group_size.*48"):
        TorchOffloadEngine([pages], cfg(fp4_group_size=48))
    with pytest.raises(ValueError, match="fp4_group_size.*256"):
        TorchOffloadEngine([pages], cfg(fp4_group_size=256))
    # 4112 bytes = 2056 elements: a multiple of 16 bytes, not of G = 32
    odd = [torch.zeros(4, 2056, dtype=torch.bfloat16)]
    with pytest.raises(ValueError, match=r"group 0.*4112.*2056.*32"):
        TorchOffloadEngine([odd], cfg())
    with pytest.raises(ValueError, match=r"group 1.*4112.*2056.*32"):
        TorchOffloadEngine([pages, odd], cfg())
    # the fp4 group size is ignored by the other modes
    TorchOffloadEngine([odd], OffloadEngineConfig(
        copy_path="host", serialize="fp8_e4m3", fp4_group_size=48))
    # mixed 16-bit float tensors: fp4 is a converting mode
    f16 = [torch.zeros(4, 2048, dtype=torch.float16)]
    with pytest.raises(ValueError, match="mix"):
        TorchOffloadEngine([pages, f16], cfg())
    with pytest.raises(ValueError, match="kv_dtype"):
        TorchOffloadEngine([f16], cfg(kv_dtype="bfloat16"))
    # the binding rejects what the wrapper rejects
    ko = ensure_offload_native()
    t = odd[0]
    groups = [([t.data_ptr()], [4112], 4112, 4)]
    with pytest.raises(ValueError, match="fp4_group_size"):
        ko.StorageOffloadEngine(groups, io_threads=1, copy_path="host",
                                serialize="fp4_e2m1_group", fp4_group_size=48)
    with pytest.raises(ValueError, match="group 0.*2056.*32"):
        ko.StorageOffloadEngine(groups, io_threads=1, copy_path="host",
                                serialize="fp4_e2m1_group")
    copier = block_copier([pages])
    with pytest.raises(ValueError, match="group_size"):
        copier.packed_bytes_fp4_group(0, 1, 48)
    slab = torch.zeros(4096, dtype=torch.uint8)
    with pytest.raises(ValueError, match="not a multiple"):
        block_copier([odd]).gather_fp4_group(0, [0], slab.data_ptr(), 32, 0)
