"""serialize="fp8_e4m3_group" on the host path: one f32 scale per
fp8_group_size elements instead of one per (block, layer) tile.

The host-mode software codec must write exactly the bytes of the torch
oracle in fp8_group_oracle.py (the HIP kernels are held to the same bytes
in test_fp8_group_gpu.py), and every group must come back within 0.07 of
its OWN amax on input whose groups span five decades — the case the
per-tile mode loses.
"""
import logging
import os
import time

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

NUM_BLOCKS = 32
NUM_LAYERS = 2
BPF = 8

# (block_bytes, group_size): every group size at 4096, and a tile that is
# no multiple of 1 KiB (384 elements = 3 groups)
CASES = [(4096, 64), (4096, 128), (4096, 256), (4096, 512), (768, 128)]


def _engine(pages, tmp, model, bb, gs, bpf=BPF, **kw):
    eng = TorchOffloadEngine(
        [pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=bpf,
                            copy_path="host", serialize="fp8_e4m3_group",
                            fp8_group_size=gs, **kw))
    mapper = FileMapper(str(tmp),
                        KVCacheLayoutConfig(model=model,
                                            dtype=f"bfloat16+fp8g{gs}"))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [bpf]),
            StorageToGPUHandler(eng, mapper, [bpf]))


@pytest.fixture(scope="module", params=CASES,
                ids=[f"bb{b}-g{g}" for b, g in CASES])
def roundtrip(request, tmp_path_factory):
    """One host-mode store + load per case, shared by the checks below."""
    bb, gs = request.param
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=bb + gs)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(
        pages, tmp_path_factory.mktemp("fp8g"), "fp8g", bb, gs)
    ids = list(range(1, 2 * BPF, 2))  # 8 odd blocks -> one file
    store.transfer_async([0x61], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0x61, 0)
    data = torch.frombuffer(bytearray(open(path, "rb").read()),
                            dtype=torch.uint8)
    for p in pages:
        p.zero_()
    load.transfer_async([0x61], {0: ids})
    assert wait_finished(load)[0].success
    return dict(bb=bb, gs=gs, ids=ids, orig=orig, pages=pages, data=data,
                eng=eng)


def test_record_bytes_in_geometry(roundtrip):
    r = roundtrip
    assert r["eng"].group_geometry[0]["record_bytes"] == \
        record_bytes(r["bb"], r["gs"])


def test_file_size_exact(roundtrip):
    r = roundtrip
    n = r["bb"] // 2
    assert r["data"].numel() == BPF * NUM_LAYERS * (n + 4 * n // r["gs"])


def test_file_bytes_equal_oracle(roundtrip):
    r = roundtrip
    want = oracle_records(r["orig"], r["ids"], r["gs"])
    assert r["data"].numel() == want.numel()
    diff = (r["data"] != want).nonzero().flatten()
    assert diff.numel() == 0, \
        f"{diff.numel()} file bytes differ from the oracle, first at {diff[:8]}"


def test_loaded_values_equal_oracle(roundtrip):
    r = roundtrip
    untouched = [i for i in range(NUM_BLOCKS) if i not in r["ids"]]
    for page, o in zip(r["pages"], r["orig"]):
        _, _, y, _ = oracle(o[r["ids"]], r["gs"])
        assert torch.equal(page[r["ids"]].view(torch.int16),
                           y.view(torch.int16))
        assert (page[untouched].view(torch.int16) == 0).all()


def test_per_group_accuracy(roundtrip):
    r = roundtrip
    for page, o in zip(r["pages"], r["orig"]):
        assert_group_bound(page[r["ids"]], o[r["ids"]], r["gs"])


def test_planted_values_survive(roundtrip):
    """+-448*s and 0.5*s in a group of amax 448*s are e4m3-exact, and an
    all-zero group stores scale 1/448 and returns zeros."""
    r = roundtrip
    ng = r["bb"] // 2 // r["gs"]
    for page, o in zip(r["pages"], r["orig"]):
        for b in r["ids"]:
            e = ((b + 1) % ng) * r["gs"]
            assert torch.equal(page[b, e:e + 3], o[b, e:e + 3])
            z = (b % ng) * r["gs"]
            assert (page[b, z:z + r["gs"]].float() == 0).all()


def test_partial_and_offset_loads(tmp_path):
    """24 blocks at 16 per file; blocks 20-23 are tail-seeked out of the
    second (short) file by record size."""
    bb, gs, bpf = 4096, 128, 16
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=7)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(pages, tmp_path, "fp8g-part", bb, gs,
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
        _, _, y, _ = oracle(o[20:24], gs)
        assert torch.equal(page[20:24].view(torch.int16), y.view(torch.int16))
        assert (page[:20].view(torch.int16) == 0).all()
        assert (page[24:].view(torch.int16) == 0).all()


def test_dram_cache_and_writeback(tmp_path):
    """Composed with the pinned cache + write-back: the flush writes the
    grouped file, and a DRAM hit serves after the file is deleted."""
    bb, gs = 4096, 128
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=11)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(
        pages, tmp_path, "fp8g-wb", bb, gs, host_cache_bytes=64 << 20,
        write_policy="back")
    ids = list(range(BPF))
    store.transfer_async([0xFB], {0: ids})
    assert wait_finished(store)[0].success
    deadline = time.time() + 10
    while eng.stats().writeback_flushes < 1 and time.time() < deadline:
        time.sleep(0.005)
    path = mapper.file_name(0xFB, 0)
    data = torch.frombuffer(bytearray(open(path, "rb").read()),
                            dtype=torch.uint8)
    assert torch.equal(data, oracle_records(orig, ids, gs))
    os.unlink(path)
    for p in pages:
        p.zero_()
    load.transfer_async([0xFB], {0: ids})
    assert wait_finished(load)[0].success
    assert eng.stats().host_cache_hits >= 1
    for page, o in zip(pages, orig):
        _, _, y, _ = oracle(o[ids], gs)
        assert torch.equal(page[ids].view(torch.int16), y.view(torch.int16))


def test_construction_errors():
    pages = [torch.zeros(4, 2048, dtype=torch.bfloat16)]
    with pytest.raises(ValueError, match="fp8_group_size.*96"):
        TorchOffloadEngine([pages], OffloadEngineConfig(
            copy_path="host", serialize="fp8_e4m3_group", fp8_group_size=96))
    # 4128 bytes = 2064 elements: a multiple of 16 bytes, not of G = 128
    odd = [torch.zeros(4, 2064, dtype=torch.bfloat16)]
    with pytest.raises(ValueError, match=r"group 0.*4128.*2064.*128"):
        TorchOffloadEngine([odd], OffloadEngineConfig(
            copy_path="host", serialize="fp8_e4m3_group"))
    # the offending group is named when it is not the first
    with pytest.raises(ValueError, match=r"group 1.*4128.*2064.*128"):
        TorchOffloadEngine([pages, odd], OffloadEngineConfig(
            copy_path="host", serialize="fp8_e4m3_group"))
    # the group size is ignored by the other modes
    TorchOffloadEngine([odd], OffloadEngineConfig(
        copy_path="host", serialize="fp8_e4m3", fp8_group_size=96))
    with pytest.raises(ValueError,
                       match=r"raw\|fp8_e4m3\|fp8_e4m3_group"):
        TorchOffloadEngine([pages], OffloadEngineConfig(
            copy_path="host", serialize="fp8_e5m2"))


def test_native_engine_validates_too():
    """The binding rejects what the Python wrapper rejects, for callers
    that construct the native engine directly."""
    from llm_d_kv_cache_amd import ensure_offload_native

    ko = ensure_offload_native()
    t = torch.zeros(4, 2064, dtype=torch.bfloat16)
    groups = [([t.data_ptr()], [4128], 4128, 4)]
    with pytest.raises(ValueError, match="fp8_group_size"):
        ko.StorageOffloadEngine(groups, io_threads=1, copy_path="host",
                                serialize="fp8_e4m3_group", fp8_group_size=96)
    with pytest.raises(ValueError, match="group 0.*2064.*128"):
        ko.StorageOffloadEngine(groups, io_threads=1, copy_path="host",
                                serialize="fp8_e4m3_group")


def test_block_copier_host_twin():
    """BlockCopier's CPU path: same bytes as the oracle, round trip equal
    to the oracle's dequantized values."""
    from llm_d_kv_cache_amd.ops import block_copier

    bb, gs = 768, 128
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=3)
    orig = [p.clone() for p in pages]
    copier = block_copier([pages])
    ids = [5, 2, 9]
    nbytes = copier.packed_bytes_fp8_group(0, len(ids), gs)
    assert nbytes == len(ids) * NUM_LAYERS * record_bytes(bb, gs)
    slab = torch.zeros(nbytes, dtype=torch.uint8)
    copier.gather_fp8_group(0, ids, slab.data_ptr(), gs, 0)
    assert torch.equal(slab, oracle_records(orig, ids, gs))
    for p in pages:
        p.zero_()
    copier.scatter_fp8_group(0, ids, slab.data_ptr(), gs, 0)
    for page, o in zip(pages, orig):
        _, _, y, _ = oracle(o[ids], gs)
        assert torch.equal(page[ids].view(torch.int16), y.view(torch.int16))
    with pytest.raises(ValueError, match="group_size"):
        copier.packed_bytes_fp8_group(0, 1, 96)
    with pytest.raises(ValueError, match="not a multiple"):
        copier.gather_fp8_group(0, ids, slab.data_ptr(), 256, 0)


def test_obj_tier_roundtrip():
    """ObjStorageEngine with the grouped codec against the in-repo fake S3:
    the object holds the oracle's bytes, a ranged partial load lands."""
    import threading

    from test_obj_backend import ThreadingHTTPServer, _FakeS3

    from llm_d_kv_cache_amd.offload.obj_backend import (
        ObjKeyMapper, ObjStorageConfig, ObjStorageEngine)

    bb, gs = 4096, 128
    _FakeS3.store = {}
    srv = ThreadingHTTPServer(("127.0.0.1", 0), _FakeS3)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        pages = make_pages(16, bb, gs, NUM_LAYERS, seed=6)
        orig = [p.clone() for p in pages]
        eng = ObjStorageEngine(
            [pages],
            ObjStorageConfig(endpoint=f"http://127.0.0.1:{srv.server_port}",
                             serialize="fp8_e4m3_group", fp8_group_size=gs))
        assert eng.group_geometry[0]["record_bytes"] == record_bytes(bb, gs)
        mapper = ObjKeyMapper(FileMapper("/kv", KVCacheLayoutConfig(
            model="objg", dtype="bfloat16+fp8g128")))
        store = GPUToStorageHandler(eng, mapper, [8])
        load = StorageToGPUHandler(eng, mapper, [8])
        ids = list(range(8))
        store.transfer_async([0xE8], {0: ids})
        assert wait_finished(store)[0].success
        (obj,) = _FakeS3.store.values()
        assert torch.equal(
            torch.frombuffer(bytearray(obj), dtype=torch.uint8),
            oracle_records(orig, ids, gs))
        for p in pages:
            p.zero_()
        load.transfer_async([0xE8], {0: [6, 7]}, skip_leading_blocks=6)
        assert wait_finished(load)[0].success
        for page, o in zip(pages, orig):
            _, _, y, _ = oracle(o[6:8], gs)
            assert torch.equal(page[6:8].view(torch.int16),
                               y.view(torch.int16))
            assert (page[:6].view(torch.int16) == 0).all()
        eng.close()
        with pytest.raises(ValueError, match="fp8_group_size"):
            ObjStorageEngine([pages], ObjStorageConfig(
                serialize="fp8_e4m3_group", fp8_group_size=100))
    finally:
        srv.shutdown()


def test_peer_dram_lookup_always_misses(tmp_path, caplog):
    """The peer wire has no grouped format: a lookup built for a grouped
    engine reports a miss for a chunk that IS resident in the DRAM tier
    (so its bytes are never labelled raw), and says so once."""
    from llm_d_kv_cache_amd.peer.tiered import make_dram_lookup

    bb, gs = 4096, 128
    pages = make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=13)
    eng, mapper, store, _ = _engine(pages, tmp_path, "fp8g-peer", bb, gs,
                                    host_cache_bytes=64 << 20)
    store.transfer_async([0x62], {0: list(range(BPF))})
    assert wait_finished(store)[0].success
    resident = eng.dram_chunk(mapper.file_name(0x62, 0), BPF, 0)
    assert resident is not None
    assert resident.numel() == BPF * NUM_LAYERS * record_bytes(bb, gs)
    lookup = make_dram_lookup(eng, mapper)
    with caplog.at_level(logging.WARNING,
                         logger="llm_d_kv_cache_amd.peer.tiered"):
        assert lookup(0x62, 0, BPF) is None
        assert lookup(0x62, 0, BPF) is None
    assert len([r for r in caplog.records
                if "fp8_e4m3_group" in r.getMessage()]) == 1
