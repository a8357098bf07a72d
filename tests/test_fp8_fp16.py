"""fp16 KV pages through both fp8 serialize modes on the host path.

The records are dtype-free; only the page -> f32 conversion on store and the
f32 -> page rounding on load depend on the page type. The host-mode codec
must write exactly the bytes of the torch oracle in fp8_fp16_oracle.py and
load exactly its values, bit for bit, fp16 subnormals and +-65504 included
(the HIP kernels are held to the same bytes in test_fp8_fp16_gpu.py), and
`kv_dtype` must resolve the same way on every entry point.
"""
import multiprocessing as mp
import os
import threading

import pytest
import torch

import checksum_oracle as co
import fp8_group_oracle as bf16_group
import fp8_tile_oracle as bf16_tile
from fp8_fp16_oracle import (
    assert_group_bound,
    bits,
    count_subnormal,
    loaded_values,
    make_group_pages,
    make_tile_pages,
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

NUM_BLOCKS = 16
NUM_LAYERS = 2
BPF = 8

# (serialize, block_bytes, group_size); group_size None = per tile (G = n).
# 768 B = 3 groups (no multiple of 1 KiB), every group size class at 4096;
# 1152 B and 8208 B are the per-tile shapes of test_fp8_tile.py (n/8 no
# multiple of 64; more than one 256-lane sweep plus a ragged tail).
CASES = [
    ("fp8_e4m3_group", 768, 128),
    ("fp8_e4m3_group", 4096, 64),
    ("fp8_e4m3_group", 4096, 512),
    ("fp8_e4m3", 1152, None),
    ("fp8_e4m3", 8208, None),
]
CASE_IDS = [f"{m}-bb{b}" + (f"-g{g}" if g else "") for m, b, g in CASES]


def _pages(case, dtype=torch.float16, num_blocks=NUM_BLOCKS, seed=None):
    mode, bb, gs = case
    seed = bb + (gs or 0) if seed is None else seed
    if gs:
        return make_group_pages(num_blocks, bb, gs, NUM_LAYERS, seed, dtype)
    return make_tile_pages(num_blocks, bb, NUM_LAYERS, seed, dtype)


def _G(case):
    return case[2] or case[1] // 2


def _engine(pages, tmp, case, model="f16", bpf=BPF, **kw):
    mode, bb, gs = case
    eng = TorchOffloadEngine(
        [pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=bpf,
                            copy_path="host", serialize=mode,
                            fp8_group_size=gs or 128, **kw))
    tag = f"{eng.kv_dtype}+{mode}" + (f"{gs}" if gs else "") + \
        ("+ck" if kw.get("checksum") else "")
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(model=model, dtype=tag))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [bpf]),
            StorageToGPUHandler(eng, mapper, [bpf]))


def _file_payloads(path, P, checksum):
    raw = open(path, "rb").read()
    if checksum:
        assert co.verify(raw, P) == (0, -1)
        raw = co.payloads(raw, P)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8)


def _assert_bytes(got, want, what):
    assert got.numel() == want.numel(), \
        f"{what}: {got.numel()} bytes, oracle has {want.numel()}"
    diff = (got != want).nonzero().flatten()
    assert diff.numel() == 0, (
        f"{what}: {diff.numel()} of {want.numel()} bytes differ from the "
        f"oracle, first at {diff[:8].tolist()}")


def _assert_loaded(pages, orig, ids, G, out_dtype=None):
    """Loaded blocks equal oracle y bit for bit, every other block is zero."""
    untouched = [i for i in range(pages[0].shape[0]) if i not in ids]
    for page, y in zip(pages, loaded_values(orig, ids, G, out_dtype)):
        got, want = bits(page[ids]), bits(y)
        bad = (got != want).sum().item()
        assert bad == 0, f"{bad} of {want.numel()} loaded values differ"
        assert (bits(page[untouched]) == 0).all()


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "ck"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_engine_host_matches_oracle(tmp_path, case, checksum):
    mode, bb, gs = case
    G = _G(case)
    orig = _pages(case)
    pages = [p.clone() for p in orig]
    eng, mapper, store, load = _engine(pages, tmp_path, case,
                                       checksum=checksum)
    assert eng.kv_dtype == "float16"
    ids = list(range(1, 2 * BPF, 2))  # 8 odd blocks -> one file
    store.transfer_async([0x61], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0x61, 0)
    P = record_bytes(bb, G)
    assert os.path.getsize(path) == \
        BPF * NUM_LAYERS * (P + (16 if checksum else 0))
    _assert_bytes(_file_payloads(path, P, checksum),
                  oracle_records(orig, ids, G), "file")
    for p in pages:
        p.zero_()
    load.transfer_async([0x61], {0: ids})
    assert wait_finished(load)[0].success
    assert eng.stats().errors == 0
    _assert_loaded(pages, orig, ids, G)
    for page, o in zip(pages, orig):
        assert torch.isfinite(page[ids].float()).all()
        assert_group_bound(page[ids], o[ids], G)
    # the load really produced fp16 subnormals
    assert sum(count_subnormal(p[ids]) for p in pages) > 0


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "ck"])
@pytest.mark.parametrize("case", [CASES[0], CASES[3]],
                         ids=[CASE_IDS[0], CASE_IDS[3]])
def test_tail_seek_partial_load(tmp_path, case, checksum):
    """12 blocks at 8 per file; blocks 10-11 are tail-seeked out of the
    second (short) file by record size."""
    mode, bb, gs = case
    G = _G(case)
    orig = _pages(case, seed=7)
    pages = [p.clone() for p in orig]
    eng, mapper, store, load = _engine(pages, tmp_path, case, model="part",
                                       checksum=checksum)
    store.transfer_async([0xB1, 0xB2], {0: list(range(12))})
    assert wait_finished(store)[0].success
    rec = record_bytes(bb, G) + (16 if checksum else 0)
    assert os.path.getsize(mapper.file_name(0xB1, 0)) == 8 * NUM_LAYERS * rec
    assert os.path.getsize(mapper.file_name(0xB2, 0)) == 4 * NUM_LAYERS * rec
    for p in pages:
        p.zero_()
    load.transfer_async([0xB1, 0xB2], {0: [10, 11]}, skip_leading_blocks=10)
    assert wait_finished(load)[0].success
    assert eng.stats().errors == 0
    _assert_loaded(pages, orig, [10, 11], G)


@pytest.mark.parametrize("case", CASES + [("fp8_e4m3", 16, None)],
                         ids=CASE_IDS + ["fp8_e4m3-bb16"])
def test_block_copier_host(case):
    from llm_d_kv_cache_amd.ops import block_copier

    mode, bb, gs = case
    G = _G(case)
    orig = _pages(case, seed=3)
    pages = [p.clone() for p in orig]
    copier = block_copier([pages])
    ids = [5, 2, 3, 9]
    want = oracle_records(orig, ids, G)
    if gs:
        nbytes = copier.packed_bytes_fp8_group(0, len(ids), gs)
    else:
        nbytes = copier.packed_bytes_fp8(0, len(ids))
    assert nbytes == want.numel()
    slab = torch.full((nbytes,), 0xA5, dtype=torch.uint8)
    if gs:
        copier.gather_fp8_group(0, ids, slab.data_ptr(), gs, 0)
    else:
        copier.gather_fp8(0, ids, slab.data_ptr(), 0, 0)
    _assert_bytes(slab, want, "slab")
    # scatter the ORACLE's bytes, so the decoder is checked on its own
    for p in pages:
        p.zero_()
    src = want.clone()
    if gs:
        copier.scatter_fp8_group(0, ids, src.data_ptr(), gs, 0)
    else:
        copier.scatter_fp8(0, ids, src.data_ptr(), 0)
    _assert_loaded(pages, orig, ids, G)


@pytest.mark.parametrize("case", [CASES[1], CASES[3]],
                         ids=[CASE_IDS[1], CASE_IDS[3]])
def test_obj_tier_roundtrip(case):
    """ObjStorageEngine against the in-repo fake S3: the object holds the
    oracle's bytes, a ranged partial load lands the oracle's values."""
    from test_obj_backend import ThreadingHTTPServer, _FakeS3

    from llm_d_kv_cache_amd.offload.obj_backend import (
        ObjKeyMapper, ObjStorageConfig, ObjStorageEngine)

    mode, bb, gs = case
    G = _G(case)
    _FakeS3.store = {}
    srv = ThreadingHTTPServer(("127.0.0.1", 0), _FakeS3)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        orig = _pages(case, seed=6)
        pages = [p.clone() for p in orig]
        eng = ObjStorageEngine(
            [pages],
            ObjStorageConfig(endpoint=f"http://127.0.0.1:{srv.server_port}",
                             serialize=mode, fp8_group_size=gs or 128))
        assert eng.kv_dtype == "float16"
        mapper = ObjKeyMapper(FileMapper("/kv", KVCacheLayoutConfig(
            model="objf16", dtype=f"float16+{mode}")))
        store = GPUToStorageHandler(eng, mapper, [8])
        load = StorageToGPUHandler(eng, mapper, [8])
        ids = list(range(8))
        store.transfer_async([0xE8], {0: ids})
        assert wait_finished(store)[0].success
        (obj,) = _FakeS3.store.values()
        _assert_bytes(torch.frombuffer(bytearray(obj), dtype=torch.uint8),
                      oracle_records(orig, ids, G), "object")
        for p in pages:
            p.zero_()
        load.transfer_async([0xE8], {0: [6, 7]}, skip_leading_blocks=6)
        assert wait_finished(load)[0].success
        _assert_loaded(pages, orig, [6, 7], G)
        eng.close()
        with pytest.raises(ValueError, match="kv_dtype"):
            ObjStorageEngine([pages], ObjStorageConfig(
                serialize=mode, kv_dtype="bfloat16"))
    finally:
        srv.shutdown()


def _store_file(pages, tmp, case, model, **kw):
    eng, mapper, store, _ = _engine(pages, tmp, case, model=model, **kw)
    ids = list(range(BPF))
    store.transfer_async([0x33], {0: ids})
    assert wait_finished(store)[0].success
    data = torch.frombuffer(
        bytearray(open(mapper.file_name(0x33, 0), "rb").read()),
        dtype=torch.uint8)
    return eng, data, ids


@pytest.mark.parametrize("case", [CASES[1], CASES[3]],
                         ids=[CASE_IDS[1], CASE_IDS[3]])
def test_auto_resolution(tmp_path, case):
    """float16 tensors -> fp16. uint8 views and bf16 tensors -> bf16, with
    bytes identical to the bf16 oracles that predate kv_dtype; an explicit
    value makes uint8 views of fp16 pages work."""
    mode, bb, gs = case
    G = _G(case)
    f16 = _pages(case)
    eng, data, ids = _store_file([p.clone() for p in f16], tmp_path / "a",
                                 case, "auto-f16")
    assert eng.kv_dtype == "float16"
    _assert_bytes(data, oracle_records(f16, ids, G), "fp16 file")

    if gs:
        bf = bf16_group.make_pages(NUM_BLOCKS, bb, gs, NUM_LAYERS, seed=5)
        bf_want = bf16_group.oracle_records(bf, ids, gs)
    else:
        bf = bf16_tile.make_tile_pages(NUM_BLOCKS, bb, NUM_LAYERS, seed=5)
        bf_want = bf16_tile.tile_records(bf, ids)
    eng, data, _ = _store_file([p.clone() for p in bf], tmp_path / "b", case,
                               "auto-bf16")
    assert eng.kv_dtype == "bfloat16"
    _assert_bytes(data, bf_want, "bf16 file")
    views = [p.clone().view(torch.uint8) for p in bf]
    eng, data, _ = _store_file(views, tmp_path / "c", case, "auto-u8")
    assert eng.kv_dtype == "bfloat16"
    _assert_bytes(data, bf_want, "uint8-view-of-bf16 file")

    # explicit override on opaque views of fp16 pages, store and load
    views = [p.clone().view(torch.uint8) for p in f16]
    eng, mapper, store, load = _engine(views, tmp_path / "d", case,
                                       model="u8-f16", kv_dtype="float16")
    assert eng.kv_dtype == "float16"
    store.transfer_async([0x34], {0: ids})
    assert wait_finished(store)[0].success
    data = torch.frombuffer(
        bytearray(open(mapper.file_name(0x34, 0), "rb").read()),
        dtype=torch.uint8)
    _assert_bytes(data, oracle_records(f16, ids, G), "uint8-view-of-fp16 file")
    for v in views:
        v.zero_()
    load.transfer_async([0x34], {0: ids})
    assert wait_finished(load)[0].success
    _assert_loaded(views, f16, ids, G)
    # ... and without it the same views are read as bf16: other bytes
    eng, data, _ = _store_file([p.clone().view(torch.uint8) for p in f16],
                               tmp_path / "e", case, "u8-auto")
    assert eng.kv_dtype == "bfloat16"
    assert not torch.equal(data, oracle_records(f16, ids, G))


def test_kv_dtype_errors():
    from llm_d_kv_cache_amd import ensure_offload_native
    from llm_d_kv_cache_amd.ops import block_copier

    f16 = [torch.zeros(4, 2048, dtype=torch.float16)]
    bf = [torch.zeros(4, 2048, dtype=torch.bfloat16)]
    u8 = [torch.zeros(4, 4096, dtype=torch.uint8)]
    for mode in ("fp8_e4m3", "fp8_e4m3_group"):
        def cfg(**kw):
            return OffloadEngineConfig(copy_path="host", serialize=mode, **kw)
        # explicit value against the tensors' own dtype, both directions
        with pytest.raises(ValueError, match="kv_dtype.*bfloat16.*float16"):
            TorchOffloadEngine([f16], cfg(kv_dtype="bfloat16"))
        with pytest.raises(ValueError, match="kv_dtype.*float16.*bfloat16"):
            TorchOffloadEngine([bf], cfg(kv_dtype="float16"))
        # mixed 16-bit float dtypes, in one group or across groups
        with pytest.raises(ValueError, match="mix"):
            TorchOffloadEngine([f16 + bf], cfg())
        with pytest.raises(ValueError, match="mix"):
            TorchOffloadEngine([f16, bf], cfg(kv_dtype="float16"))
        with pytest.raises(ValueError, match="auto.*bfloat16.*float16"):
            TorchOffloadEngine([f16], cfg(kv_dtype="half"))
        # agreeing and opaque combinations construct
        assert TorchOffloadEngine(
            [f16], cfg(kv_dtype="float16")).kv_dtype == "float16"
        assert TorchOffloadEngine(
            [bf], cfg(kv_dtype="bfloat16")).kv_dtype == "bfloat16"
        assert TorchOffloadEngine(
            [f16, u8], cfg(kv_dtype="float16")).kv_dtype == "float16"
        # float16 next to opaque views: not every tensor is float16
        assert TorchOffloadEngine([f16, u8], cfg()).kv_dtype == "bfloat16"
    # raw ignores the field
    raw = OffloadEngineConfig(copy_path="host", kv_dtype="bfloat16")
    TorchOffloadEngine([f16], raw)
    TorchOffloadEngine([f16, bf], OffloadEngineConfig(copy_path="host"))

    with pytest.raises(ValueError, match="kv_dtype"):
        block_copier([f16], kv_dtype="bfloat16")
    with pytest.raises(ValueError, match="kv_dtype"):
        block_copier([f16], kv_dtype="fp16")
    ko = ensure_offload_native()
    groups = [([f16[0].data_ptr()], [4096], 4096, 4)]
    with pytest.raises(ValueError, match="kv_dtype"):
        ko.BlockCopier(groups, False, 0, kv_dtype="half")
    with pytest.raises(ValueError, match="kv_dtype"):
        ko.StorageOffloadEngine(groups, io_threads=1, copy_path="host",
                                serialize="fp8_e4m3", kv_dtype="fp16")
    ko.BlockCopier(groups, False, 0, kv_dtype="float16")


@pytest.mark.parametrize("written", [torch.float16, torch.bfloat16],
                         ids=["f16-file", "bf16-file"])
@pytest.mark.parametrize("case", [CASES[0], CASES[3]],
                         ids=[CASE_IDS[0], CASE_IDS[3]])
def test_cross_dtype_load(tmp_path, case, written):
    """A record is T-free on load: a file written from fp16 pages loaded by
    a bf16 engine yields bf16_RNE(f32(q) * scale), and the reverse."""
    mode, bb, gs = case
    G = _G(case)
    other = torch.bfloat16 if written == torch.float16 else torch.float16
    orig = _pages(case, dtype=written, seed=21)
    if written == torch.bfloat16:
        # keep 448 * scale inside fp16: the loader's type bounds the range
        orig = [p.float().clamp(-60000.0, 60000.0).to(written) for p in orig]
    src = [p.clone() for p in orig]
    # both engines share one directory and one dtype tag on purpose
    mapper = FileMapper(str(tmp_path), KVCacheLayoutConfig(
        model="cross", dtype="x16+" + mode))
    cfg = OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=BPF,
                              copy_path="host", serialize=mode,
                              fp8_group_size=gs or 128)
    weng = TorchOffloadEngine([src], cfg)
    ids = list(range(BPF))
    store = GPUToStorageHandler(weng, mapper, [BPF])
    store.transfer_async([0x44], {0: ids})
    assert wait_finished(store)[0].success
    dst = [torch.zeros_like(p, dtype=other) for p in orig]
    reng = TorchOffloadEngine([dst], cfg)
    assert {weng.kv_dtype, reng.kv_dtype} == {"float16", "bfloat16"}
    load = StorageToGPUHandler(reng, mapper, [BPF])
    load.transfer_async([0x44], {0: ids})
    assert wait_finished(load)[0].success
    _assert_loaded(dst, orig, ids, G, out_dtype=other)
    for page in dst:
        assert torch.isfinite(page[ids].float()).all()


# ---- world-2 gloo peer pull --------------------------------------------------

PEER_BB, PEER_NL, PEER_NB = 1152, 2, 16


def _peer_pages(rank):
    return make_tile_pages(PEER_NB, PEER_BB, PEER_NL, seed=500 + rank)


def _peer_rank(rank, init_file, q):
    try:
        import torch.distributed as dist

        dist.init_process_group("gloo", init_method=f"file://{init_file}",
                                rank=rank, world_size=2)
        from llm_d_kv_cache_amd.peer import PeerMigrationService

        ctrl_pg = dist.new_group(backend="gloo")
        data_pg = dist.new_group(backend="gloo")
        pages = _peer_pages(rank)
        # rank 0 hands the service real fp16 tensors (auto), rank 1 opaque
        # views with the explicit value
        if rank == 0:
            svc = PeerMigrationService([pages], data_group=data_pg,
                                       control_group=ctrl_pg)
        else:
            pages = [p.view(torch.uint8) for p in pages]
            svc = PeerMigrationService([pages], data_group=data_pg,
                                       control_group=ctrl_pg,
                                       kv_dtype="float16")
        assert svc.kv_dtype == "float16"
        other = 1 - rank
        src_ids = [1, 2, 3, 5]   # zero, plain, subnormal and +-65504 tiles
        svc.register_blocks(0x51 + rank, 0, src_ids)
        dist.barrier()
        want = loaded_values(_peer_pages(other), src_ids, PEER_BB // 2)
        before = svc.stats().bytes_received
        assert svc.pull(0x51 + other, 0, [10, 11, 12, 13], src_rank=other,
                        fp8=True).result(timeout=60) is True
        assert svc.stats().bytes_received - before == \
            len(src_ids) * PEER_NL * record_bytes(PEER_BB, PEER_BB // 2)
        for page, y in zip(pages, want):
            assert torch.equal(bits(page[10:14]), bits(y))
        res = svc.pull_many([(0x51 + other, 0, [6, 7, 8, 9]), (0x9E9E, 0, [4])],
                            src_rank=other, fp8=True).result(timeout=60)
        assert res == [True, False]
        for page, y in zip(pages, want):
            assert torch.equal(bits(page[6:10]), bits(y))
        dist.barrier()
        svc.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"FAIL: {e}\n{traceback.format_exc()}"))


def test_peer_fp8_pull_of_fp16_pages(tmp_path):
    """fp8=True pulls between two ranks holding fp16 pages land the
    oracle's y per tile, bit for bit, with no protocol change."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_peer_rank,
                         args=(r, str(tmp_path / "pg_init"), q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
    assert all(v == "ok" for v in results.values()), results
