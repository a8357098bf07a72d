"""checksum=True on the host path: a 16-byte footer behind every (block,
layer) record, sealed on store and verified before a load touches a page.

The host twin must write exactly the bytes of the numpy oracle in
checksum_oracle.py (the HIP kernels are held to the same bytes in
test_checksum_gpu.py). Every corruption below must fail the load with no
page written, count in checksum_failures, and remove the poisoned file so a
later store of the key writes a fresh one.

"Two whole records exchanged" swaps the payloads of two records and leaves
each footer where it was (a record written to, or read from, the wrong
slot). Exchanging two sealed [payload | footer] units is NOT detectable by
this format: the sum mixes in the word index, not the record's position in
the file (docs/limitations.md).
"""
import logging
import os

import numpy as np
import pytest
import torch

import checksum_oracle as co
from checksum_oracle import wait_finished
from llm_d_kv_cache_amd.offload import (
    FileMapper,
    GPUToStorageHandler,
    KVCacheLayoutConfig,
    OffloadEngineConfig,
    StorageToGPUHandler,
    TorchOffloadEngine,
    record_checksum,
    tile_record_bytes,
)

NUM_BLOCKS = 32
NUM_LAYERS = 2
BPF = 8
GROUP = 128
MODES = ["raw", "fp8_e4m3", "fp8_e4m3_group"]
LAYOUT_CASES = [(m, bb) for m in MODES for bb in (768, 4096)]
SENTINEL = 0x5A5A


def make_pages(block_bytes, seed, num_blocks=NUM_BLOCKS):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(num_blocks, block_bytes // 2, generator=gen)
            .to(torch.bfloat16) for _ in range(NUM_LAYERS)]


def _tag(serialize, checksum):
    tag = "bfloat16" if serialize == "raw" else f"bfloat16+{serialize}"
    return tag + ("+ck" if checksum else "")


def _engine(pages, root, serialize="raw", checksum=True, bpf=BPF, **kw):
    eng = TorchOffloadEngine(
        [pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=bpf,
                            copy_path="host", serialize=serialize,
                            fp8_group_size=GROUP, checksum=checksum, **kw))
    mapper = FileMapper(str(root), KVCacheLayoutConfig(
        model="ck", dtype=_tag(serialize, checksum)))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [bpf]),
            StorageToGPUHandler(eng, mapper, [bpf]))


def _bits(t):
    return t.view(torch.int16)


def _fill(pages, value=SENTINEL):
    for p in pages:
        _bits(p).fill_(value)


# ---- golden values ----------------------------------------------------------

@pytest.mark.parametrize("payload,want", co.GOLDEN,
                         ids=[f"{len(p)}B" for p, _ in co.GOLDEN])
def test_golden_values(payload, want):
    assert co.checksum_python(payload) == want
    assert co.checksum(payload) == want
    assert record_checksum(payload) == want
    assert record_checksum(np.frombuffer(payload, dtype=np.uint8)) == want


def test_record_checksum_rejects_odd_length():
    with pytest.raises(ValueError, match="multiple of 4"):
        record_checksum(bytes(6))


def test_tile_record_bytes_adds_footer():
    for mode in MODES:
        plain = tile_record_bytes(mode, 4096, GROUP)
        assert plain == co.payload_bytes(mode, 4096)
        assert tile_record_bytes(mode, 4096, GROUP, checksum=True) == plain + 16
        assert plain % 4 == 0


# ---- file layout ------------------------------------------------------------

@pytest.fixture(scope="module", params=LAYOUT_CASES,
                ids=[f"{m}-bb{b}" for m, b in LAYOUT_CASES])
def layout(request, tmp_path_factory):
    """The same pages stored by a checksum=False and a checksum=True engine,
    then loaded back through each."""
    mode, bb = request.param
    root = tmp_path_factory.mktemp("cklayout")
    ids = list(range(1, 2 * BPF, 2))
    out = {}
    for ck in (False, True):
        pages = make_pages(bb, seed=bb)
        eng, mapper, store, load = _engine(pages, root, mode, ck)
        store.transfer_async([0x61], {0: ids})
        assert wait_finished(store)[0].success
        data = open(mapper.file_name(0x61, 0), "rb").read()
        for p in pages:
            p.zero_()
        load.transfer_async([0x61], {0: ids})
        assert wait_finished(load)[0].success
        out[ck] = dict(data=data, pages=pages, eng=eng)
    return dict(mode=mode, bb=bb, ids=ids, orig=make_pages(bb, seed=bb),
                plain=out[False], sealed=out[True])


def test_file_size_and_geometry(layout):
    P = co.payload_bytes(layout["mode"], layout["bb"])
    assert len(layout["plain"]["data"]) == BPF * NUM_LAYERS * P
    assert len(layout["sealed"]["data"]) == BPF * NUM_LAYERS * (P + 16)
    assert layout["sealed"]["eng"].group_geometry[0]["record_bytes"] == P + 16
    assert layout["plain"]["eng"].group_geometry[0]["record_bytes"] == P


def test_payloads_equal_plain_file(layout):
    P = co.payload_bytes(layout["mode"], layout["bb"])
    assert co.payloads(layout["sealed"]["data"], P) == layout["plain"]["data"]


def test_footers_equal_oracle(layout):
    P = co.payload_bytes(layout["mode"], layout["bb"])
    want = co.seal(layout["plain"]["data"], P)
    got = layout["sealed"]["data"]
    assert len(got) == len(want)
    diff = np.nonzero(np.frombuffer(got, np.uint8)
                      != np.frombuffer(want, np.uint8))[0]
    assert diff.size == 0, \
        f"{diff.size} file bytes differ from the oracle, first at {diff[:8]}"
    assert co.verify(got, P) == (0, -1)


def test_load_restores_pages(layout):
    ids = layout["ids"]
    others = [i for i in range(NUM_BLOCKS) if i not in ids]
    for got, plain, orig in zip(layout["sealed"]["pages"],
                                layout["plain"]["pages"], layout["orig"]):
        if layout["mode"] == "raw":
            assert torch.equal(_bits(got[ids]), _bits(orig[ids]))
        assert torch.equal(_bits(got[ids]), _bits(plain[ids]))
        assert (_bits(got[others]) == 0).all()
    st = layout["sealed"]["eng"].stats()
    assert st.checksum_failures == 0 and st.errors == 0


# ---- corruption matrix ------------------------------------------------------

CK_BB = 768
CK_P = CK_BB            # raw payload
CK_STRIDE = CK_P + 16
CK_TILES = BPF * NUM_LAYERS


def _flip(buf, byte, bit=0):
    buf[byte] ^= 1 << bit


def _swap_words(buf):
    """Exchange two unequal payload words of record 3."""
    base = 3 * CK_STRIDE
    for a in range(0, CK_P - 4, 4):
        wa, wb = buf[base + a:base + a + 4], buf[base + a + 4:base + a + 8]
        if wa != wb:
            buf[base + a:base + a + 4] = wb
            buf[base + a + 4:base + a + 8] = wa
            return
    raise AssertionError("record 3 holds one repeated word")


def _swap_records(buf):
    a, b = 2 * CK_STRIDE, 5 * CK_STRIDE
    pa, pb = bytes(buf[a:a + CK_P]), bytes(buf[b:b + CK_P])
    assert pa != pb
    buf[a:a + CK_P], buf[b:b + CK_P] = pb, pa


def _zero_record(buf):
    buf[4 * CK_STRIDE:5 * CK_STRIDE] = bytes(CK_STRIDE)


LAST = (CK_TILES - 1) * CK_STRIDE
CORRUPTIONS = {
    "first-payload-word-of-record-0": lambda b: _flip(b, 1, 3),
    "last-payload-word-of-last-record": lambda b: _flip(b, LAST + CK_P - 1, 7),
    "sum": lambda b: _flip(b, 6 * CK_STRIDE + CK_P + 5, 2),
    "magic": lambda b: _flip(b, 1 * CK_STRIDE + CK_P + 9, 0),
    "payload-bytes": lambda b: _flip(b, 7 * CK_STRIDE + CK_P + 12, 4),
    "two-words-swapped": _swap_words,
    "record-zeroed": _zero_record,
    "two-records-exchanged": _swap_records,
}


@pytest.fixture(scope="module")
def good_file(tmp_path_factory):
    """Bytes of one good checksummed raw file (8 blocks x 2 layers x 768 B)."""
    pages = make_pages(CK_BB, seed=5)
    eng, mapper, store, _ = _engine(pages, tmp_path_factory.mktemp("ckgood"))
    store.transfer_async([0xC0], {0: list(range(BPF))})
    assert wait_finished(store)[0].success
    data = open(mapper.file_name(0xC0, 0), "rb").read()
    assert co.verify(data, CK_P) == (0, -1)
    return data


@pytest.mark.parametrize("case", list(CORRUPTIONS))
def test_corruption_is_refused(tmp_path, good_file, case):
    buf = bytearray(good_file)
    CORRUPTIONS[case](buf)
    assert bytes(buf) != good_file
    assert co.verify(buf, CK_P)[0] >= 1

    orig = make_pages(CK_BB, seed=5)
    pages = make_pages(CK_BB, seed=5)
    eng, mapper, store, load = _engine(pages, tmp_path)
    path = mapper.file_name(0xC0, 0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(buf)
    ids = list(range(BPF))
    _fill(pages)
    load.transfer_async([0xC0], {0: ids})
    assert wait_finished(load)[0].success is False
    for p in pages:
        assert (_bits(p) == SENTINEL).all(), "a page was written"
    st = eng.stats()
    assert st.checksum_failures >= 1
    assert st.checksum_failures == co.verify(buf, CK_P)[0]
    assert not os.path.exists(path)

    # the key is usable again: a fresh store writes a good file
    for p, o in zip(pages, orig):
        p.copy_(o)
    store.transfer_async([0xC0], {0: ids})
    assert wait_finished(store)[0].success
    assert open(path, "rb").read() == good_file
    _fill(pages)
    load.transfer_async([0xC0], {0: ids})
    assert wait_finished(load)[0].success
    for p, o in zip(pages, orig):
        assert torch.equal(_bits(p[ids]), _bits(o[ids]))
        assert (_bits(p[BPF:]) == SENTINEL).all()


def test_failure_log_names_file_and_tile(tmp_path, good_file, capfd):
    buf = bytearray(good_file)
    _flip(buf, 5 * CK_STRIDE + 40)
    pages = make_pages(CK_BB, seed=5)
    eng, mapper, _, load = _engine(pages, tmp_path)
    path = mapper.file_name(0xC0, 0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(buf)
    load.transfer_async([0xC0], {0: list(range(BPF))})
    assert wait_finished(load)[0].success is False
    err = capfd.readouterr().err
    assert path in err and "first bad tile 5" in err


# ---- partial load -----------------------------------------------------------

@pytest.mark.parametrize("where,ok", [("outside", True), ("inside", False)])
def test_partial_load_checks_only_its_span(tmp_path, where, ok):
    """24 blocks at 16 per file, then blocks 20-23 with
    skip_leading_blocks=20: only records of the requested span count."""
    bb, bpf = 768, 16
    pages = make_pages(bb, seed=9)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(pages, tmp_path, bpf=bpf)
    store.transfer_async([0xB1, 0xB2], {0: list(range(24))})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0xB2, 0)   # blocks 16..23, 8 slots
    stride = bb + 16
    assert os.path.getsize(path) == 8 * NUM_LAYERS * stride
    # slot 4 = block 20 is the first of the span; slot 3 lies before it
    slot = 3 if where == "outside" else 5
    buf = bytearray(open(path, "rb").read())
    _flip(buf, (slot * NUM_LAYERS + 1) * stride + 100)
    with open(path, "wb") as f:
        f.write(buf)
    _fill(pages)
    load.transfer_async([0xB1, 0xB2], {0: list(range(20, 24))},
                        skip_leading_blocks=20)
    assert wait_finished(load)[0].success is ok
    for p, o in zip(pages, orig):
        if ok:
            assert torch.equal(_bits(p[20:24]), _bits(o[20:24]))
        else:
            assert (_bits(p[20:24]) == SENTINEL).all()
        assert (_bits(p[:20]) == SENTINEL).all()
        assert (_bits(p[24:]) == SENTINEL).all()
    assert (eng.stats().checksum_failures == 0) is ok
    assert os.path.exists(path) is ok


# ---- DRAM tier --------------------------------------------------------------

def test_dram_hit_after_file_deleted(tmp_path):
    pages = make_pages(CK_BB, seed=11)
    orig = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(pages, tmp_path,
                                       host_cache_bytes=8 << 20)
    ids = list(range(BPF))
    store.transfer_async([0xD1], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0xD1, 0)
    resident = eng.dram_chunk(path, BPF, 0)
    assert resident is not None
    assert bytes(resident.numpy()) == open(path, "rb").read()
    os.unlink(path)
    _fill(pages)
    load.transfer_async([0xD1], {0: ids})
    assert wait_finished(load)[0].success
    st = eng.stats()
    assert st.host_cache_hits == 1 and st.checksum_failures == 0
    for p, o in zip(pages, orig):
        assert torch.equal(_bits(p[ids]), _bits(o[ids]))


def test_dram_miss_on_corrupt_file_leaves_no_entry(tmp_path, good_file):
    """The file is corrupt before the engine ever saw the key: the miss
    load fails and nothing becomes resident."""
    buf = bytearray(good_file)
    _flip(buf, 9 * CK_STRIDE + 8)
    pages = make_pages(CK_BB, seed=5)
    eng, mapper, _, load = _engine(pages, tmp_path, host_cache_bytes=8 << 20)
    path = mapper.file_name(0xC0, 0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(buf)
    _fill(pages)
    load.transfer_async([0xC0], {0: list(range(BPF))})
    assert wait_finished(load)[0].success is False
    assert eng.dram_chunk(path, BPF, 0) is None
    assert eng.stats().checksum_failures == 1
    assert not os.path.exists(path)
    for p in pages:
        assert (_bits(p) == SENTINEL).all()


# ---- cross-mode read --------------------------------------------------------

def test_checksum_engine_refuses_plain_file(tmp_path):
    pages = make_pages(CK_BB, seed=13)
    _, pm, pstore, _ = _engine(pages, tmp_path / "plain", checksum=False)
    ids = list(range(BPF))
    pstore.transfer_async([0xE1], {0: ids})
    assert wait_finished(pstore)[0].success
    plain = open(pm.file_name(0xE1, 0), "rb").read()

    eng, mapper, _, load = _engine(pages, tmp_path / "ck")
    path = mapper.file_name(0xE1, 0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    # long enough to cover the span, so only the footers can object
    with open(path, "wb") as f:
        f.write(plain + bytes(CK_TILES * 16))
    _fill(pages)
    load.transfer_async([0xE1], {0: ids})
    assert wait_finished(load)[0].success is False
    assert eng.stats().checksum_failures >= 1
    for p in pages:
        assert (_bits(p) == SENTINEL).all()


# ---- BlockCopier ------------------------------------------------------------

def test_block_copier_host_twin():
    from llm_d_kv_cache_amd.ops import block_copier

    pages = make_pages(CK_BB, seed=3)
    orig = [p.clone() for p in pages]
    copier = block_copier([pages])
    ids = [5, 2, 9]
    tiles = len(ids) * NUM_LAYERS

    def run(P, nbytes_plain, nbytes, gather, scatter):
        assert nbytes == nbytes_plain + tiles * 16 == tiles * (P + 16)
        plain = torch.zeros(nbytes_plain, dtype=torch.uint8)
        gather(plain, False)
        slab = torch.full((nbytes,), 0xA5, dtype=torch.uint8)
        gather(slab, True)
        copier.seal_records(slab.data_ptr(), tiles, P, 0)
        want = co.seal(bytes(plain.numpy()), P)
        assert bytes(slab.numpy()) == want
        assert copier.verify_records(slab.data_ptr(), tiles, P, 0) == (0, -1)
        # one byte of record 4, then also one of record 1
        slab[4 * (P + 16) + P - 1] ^= 0x10
        assert copier.verify_records(slab.data_ptr(), tiles, P, 0) == (1, 4)
        slab[1 * (P + 16) + P + 3] ^= 0x01
        assert copier.verify_records(slab.data_ptr(), tiles, P, 0) == (2, 1)
        # scatter with the stride restores what the plain slab restores
        slab = torch.frombuffer(bytearray(want), dtype=torch.uint8)
        for p in pages:
            p.zero_()
        scatter(plain, False)
        ref = [p.clone() for p in pages]
        for p in pages:
            p.zero_()
        scatter(slab, True)
        for p, r in zip(pages, ref):
            assert torch.equal(_bits(p), _bits(r))
        for p, o in zip(pages, orig):
            p.copy_(o)

    run(CK_BB, copier.packed_bytes(0, len(ids)),
        copier.packed_bytes(0, len(ids), checksum=True),
        lambda s, ck: copier.gather(0, ids, s.data_ptr(), 0, checksum=ck),
        lambda s, ck: copier.scatter(0, ids, s.data_ptr(), 0, checksum=ck))
    run(CK_BB // 2 + 4, copier.packed_bytes_fp8(0, len(ids)),
        copier.packed_bytes_fp8(0, len(ids), checksum=True),
        lambda s, ck: copier.gather_fp8(0, ids, s.data_ptr(), 0, 0,
                                        checksum=ck),
        lambda s, ck: copier.scatter_fp8(0, ids, s.data_ptr(), 0,
                                         checksum=ck))
    run(co.payload_bytes("fp8_e4m3_group", CK_BB),
        copier.packed_bytes_fp8_group(0, len(ids), GROUP),
        copier.packed_bytes_fp8_group(0, len(ids), GROUP, checksum=True),
        lambda s, ck: copier.gather_fp8_group(0, ids, s.data_ptr(), GROUP, 0,
                                              checksum=ck),
        lambda s, ck: copier.scatter_fp8_group(0, ids, s.data_ptr(), GROUP, 0,
                                               checksum=ck))
    with pytest.raises(ValueError, match="multiple of 4"):
        copier.seal_records(pages[0].data_ptr(), 1, 6, 0)


# ---- peer DRAM serving ------------------------------------------------------

def test_peer_dram_lookup_always_misses(tmp_path, caplog):
    from llm_d_kv_cache_amd.peer.tiered import make_dram_lookup

    pages = make_pages(CK_BB, seed=17)
    eng, mapper, store, _ = _engine(pages, tmp_path, host_cache_bytes=8 << 20)
    store.transfer_async([0x62], {0: list(range(BPF))})
    assert wait_finished(store)[0].success
    assert eng.dram_chunk(mapper.file_name(0x62, 0), BPF, 0) is not None
    lookup = make_dram_lookup(eng, mapper)
    with caplog.at_level(logging.WARNING,
                         logger="llm_d_kv_cache_amd.peer.tiered"):
        assert lookup(0x62, 0, BPF) is None
        assert lookup(0x62, 0, BPF) is None
    assert len([r for r in caplog.records
                if "checksum" in r.getMessage()]) == 1
