"""checksum=True through the HIP kernels on MI355X.

kvc_seal_records / kvc_verify_records must agree bit for bit with the numpy
oracle (checksum_oracle.py) and with host mode (test_checksum.py), so files
move freely between GPU and host-mode engines. Shapes are the smallest at
which the kernels can still go wrong:

  raw   768 B x 2 x 4      P = 768: a partly filled wave, one workgroup
  fp8   768 B x 2 x 4      P = 388 = 24*16 + 4, stride 404: every record
                           after the first is only 4-byte aligned (head
                           words peeled) and has a tail of odd words
  fp8g  8448 B x 2 x 4     P = 4356 = 272*16 + 4: several slices per tile
  raw   64 KiB x 4 x 16    many slices: partial sums across workgroups
  raw   768 B x 2 x 160    ids through the device id buffer, 320 tiles
"""
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
)

pytestmark = pytest.mark.gpu

GROUP = 128
# (serialize, block_bytes, num_layers, blocks == blocks per file)
SHAPES = [
    ("raw", 768, 2, 4),
    ("fp8_e4m3", 768, 2, 4),
    ("fp8_e4m3_group", 8448, 2, 4),
    ("raw", 65536, 4, 16),
    ("raw", 768, 2, 160),
]
SHAPE_IDS = [f"{m}-bb{b}-l{l}-n{n}" for m, b, l, n in SHAPES]

_inputs = {}


def _e4m3_exact_pages(num_blocks, n, nl, gen):
    """bf16 pages whose values are e4m3 values times 2^-3, every tile
    holding +-448 * 2^-3: the tile scale is exactly 2^-3 and every scaled
    value is an fp8 value, so no encoder has anything to round."""
    pages = []
    for _ in range(nl):
        codes = torch.randint(0, 256, (num_blocks, n), generator=gen,
                              dtype=torch.int64).to(torch.uint8)
        codes[(codes & 0x7F) == 0x7F] = 0x3A      # NaN codes
        codes[codes == 0x80] = 0x00               # -0
        codes[:, 5] = 0x7E                        # +448
        codes[:, n - 1] = 0xFE                    # -448, in the tail word
        x = codes.view(torch.float8_e4m3fn).float() * 0.125
        pages.append(x.to(torch.bfloat16))
    return pages


def cpu_pages(shape):
    """CPU pages of one shape and the ids the tests move (the odd blocks);
    computed once, shared read-only.

    The per-tile fp8 shape uses values that quantize exactly, so the byte
    comparison with host mode here rests on the footers alone. (Host mode
    and v_cvt_pk_fp8_f32 also agree on general input, ties included:
    test_fp8_tile_gpu.py holds both to one oracle.)"""
    if shape not in _inputs:
        mode, bb, nl, nb = shape
        gen = torch.Generator().manual_seed(bb + nl + nb)
        if mode == "fp8_e4m3":
            pages = _e4m3_exact_pages(2 * nb + 2, bb // 2, nl, gen)
        else:
            pages = [torch.randn(2 * nb + 2, bb // 2, generator=gen)
                     .to(torch.bfloat16) for _ in range(nl)]
        ids = list(range(1, 2 * nb, 2))
        _inputs[shape] = (pages, ids)
    return _inputs[shape]


def _tag(mode, checksum):
    tag = "bfloat16" if mode == "raw" else f"bfloat16+{mode}"
    return tag + ("+ck" if checksum else "")


def _engine(pages, tmp, shape, copy_path, checksum=True, **kw):
    mode, bb, nl, nb = shape
    eng = TorchOffloadEngine(
        [pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=nb,
                            copy_path=copy_path, serialize=mode,
                            fp8_group_size=GROUP, checksum=checksum, **kw))
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(
        model=f"gck-{copy_path}", dtype=_tag(mode, checksum)))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [nb]),
            StorageToGPUHandler(eng, mapper, [nb]))


def _assert_bytes(got, want, what):
    got = np.frombuffer(bytes(got), np.uint8)
    want = np.frombuffer(bytes(want), np.uint8)
    assert got.size == want.size, \
        f"{what}: {got.size} bytes, expected {want.size}"
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, (
        f"{what}: {diff.size} bytes differ, first offsets {diff[:8].tolist()}")


def _raw_plain(pages, ids):
    """Block-major, layer-minor raw gather of CPU pages."""
    return b"".join(bytes(p[b].view(torch.uint8).numpy())
                    for b in ids for p in pages)


def _roundtrip(dev_pages, tmp, shape, copy_path, checksum, key):
    """Store + zeroed load through a GPU engine: (file bytes, loaded pages
    on the CPU, stats)."""
    pages, ids = cpu_pages(shape)
    eng, mapper, store, load = _engine(dev_pages, tmp, shape, copy_path,
                                       checksum)
    for d, p in zip(dev_pages, pages):
        d.copy_(p)
    torch.cuda.synchronize()
    store.transfer_async([key], {0: ids})
    assert wait_finished(store)[0].success
    data = open(mapper.file_name(key, 0), "rb").read()
    for d in dev_pages:
        d.zero_()
    torch.cuda.synchronize()
    load.transfer_async([key], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    return data, [d.cpu() for d in dev_pages], eng.stats()


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_gpu_engine_roundtrip(tmp_path, shape, copy_path):
    """The checksummed file is the checksum=False file of the same engine
    with the oracle's footers added (for raw: the oracle's file outright),
    and it loads back to the same pages."""
    mode, bb, nl, nb = shape
    pages, ids = cpu_pages(shape)
    P = co.payload_bytes(mode, bb)
    dev_pages = [p.cuda() for p in pages]
    plain, want, _ = _roundtrip(dev_pages, tmp_path / "plain", shape,
                                copy_path, False, 0x72)
    data, loaded, st = _roundtrip(dev_pages, tmp_path / "ck", shape, copy_path,
                                  True, 0x71)
    assert len(plain) == nb * nl * P
    assert len(data) == nb * nl * (P + 16)
    _assert_bytes(co.payloads(data, P), plain, "payloads/plain file")
    _assert_bytes(data, co.seal(plain, P), "file/oracle over plain file")
    if mode == "raw":
        _assert_bytes(data, co.seal(_raw_plain(pages, ids), P), "file/oracle")
        want = pages
    assert st.checksum_failures == 0 and st.errors == 0
    others = [i for i in range(2 * nb + 2) if i not in set(ids)]
    for got, w in zip(loaded, want):
        assert torch.equal(got[ids].view(torch.int16),
                           w[ids].view(torch.int16))
        assert (got[others].view(torch.int16) == 0).all()


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_gpu_file_equals_host_mode_file(tmp_path, shape, copy_path):
    """Byte for byte the file a host-mode engine writes for the same CPU
    pages.

    The per-tile fp8 shape runs on exactly quantizable pages (see
    cpu_pages); general input is compared in test_fp8_tile_gpu.py.
    """
    mode, bb, nl, nb = shape
    pages, ids = cpu_pages(shape)
    P = co.payload_bytes(mode, bb)
    host_pages = [p.clone() for p in pages]
    _, hm, hstore, _ = _engine(host_pages, tmp_path / "host", shape, "host")
    hstore.transfer_async([0x71], {0: ids})
    assert wait_finished(hstore)[0].success
    host_file = open(hm.file_name(0x71, 0), "rb").read()
    assert co.verify(host_file, P) == (0, -1)

    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, _ = _engine(dev_pages, tmp_path / "ck", shape,
                                    copy_path)
    store.transfer_async([0x71], {0: ids})
    assert wait_finished(store)[0].success
    data = open(mapper.file_name(0x71, 0), "rb").read()
    assert co.verify(data, P) == (0, -1)
    _assert_bytes(data, host_file, "file/host mode")


def _device_slab(shape):
    """Gather with stride into a 0xA5 slab with a 256-byte guard band, seal
    it: (copier, slab, tiles, P, expected bytes)."""
    from llm_d_kv_cache_amd.ops import block_copier

    mode, bb, nl, nb = shape
    pages, ids = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    copier = block_copier([dev_pages])
    stream = torch.cuda.current_stream().cuda_stream
    tiles = len(ids) * nl
    P = co.payload_bytes(mode, bb)
    if mode == "raw":
        nplain = copier.packed_bytes(0, len(ids))
        nbytes = copier.packed_bytes(0, len(ids), checksum=True)

        def gather(s, ck):
            copier.gather(0, ids, s.data_ptr(), stream, checksum=ck)
    else:
        assert mode == "fp8_e4m3"
        nplain = copier.packed_bytes_fp8(0, len(ids))
        nbytes = copier.packed_bytes_fp8(0, len(ids), checksum=True)
        scratch = torch.empty(copier.fp8_scratch_bytes(0, len(ids)),
                              dtype=torch.uint8, device="cuda")

        def gather(s, ck):
            copier.gather_fp8(0, ids, s.data_ptr(), scratch.data_ptr(),
                              stream, checksum=ck)
    assert nplain == tiles * P and nbytes == tiles * (P + 16)
    plain = torch.empty(nplain, dtype=torch.uint8, device="cuda")
    gather(plain, False)
    slab = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    gather(slab, True)
    copier.seal_records(slab.data_ptr(), tiles, P, stream)
    torch.cuda.synchronize()
    want = co.seal(bytes(plain.cpu().numpy()), P)
    if mode == "raw":
        assert want == co.seal(_raw_plain(pages, ids), P)
    return copier, slab, tiles, P, want, dev_pages


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[1], SHAPES[0]],
                         ids=[SHAPE_IDS[3], SHAPE_IDS[1], SHAPE_IDS[0]])
def test_gpu_block_copier_seal_and_verify(shape):
    copier, slab, tiles, P, want, _keep = _device_slab(shape)
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = tiles * (P + 16)
    host = slab.cpu().numpy()
    _assert_bytes(host[:nbytes], want, "sealed slab")
    assert (host[nbytes:] == 0xA5).all(), "guard band overwritten"
    assert copier.verify_records(slab.data_ptr(), tiles, P, stream) == (0, -1)
    # verify is read-only
    assert bytes(slab.cpu().numpy()) == bytes(host)

    # one bit in the LAST payload word of a record: at 64 KiB a word owned
    # by the last slice, at 388 bytes the 4-byte tail behind the vectors
    rec = tiles - 3
    idx = rec * (P + 16) + P - 2
    slab[idx] = slab[idx] ^ 0x40
    assert copier.verify_records(slab.data_ptr(), tiles, P, stream) == (1, rec)
    # ... and one in the first word of an earlier record
    idx0 = 1 * (P + 16) + 1
    slab[idx0] = slab[idx0] ^ 0x01
    assert copier.verify_records(slab.data_ptr(), tiles, P, stream) == (2, 1)
    # sealing again repairs every footer, whatever it held
    copier.seal_records(slab.data_ptr(), tiles, P, stream)
    assert copier.verify_records(slab.data_ptr(), tiles, P, stream) == (0, -1)
    assert (slab[nbytes:].cpu() == 0xA5).all(), "guard band overwritten"


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
def test_gpu_corrupt_file_is_refused(tmp_path, copy_path):
    shape = SHAPES[0]
    mode, bb, nl, nb = shape
    pages, ids = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(dev_pages, tmp_path, shape, copy_path)
    store.transfer_async([0xBD], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0xBD, 0)
    buf = bytearray(open(path, "rb").read())
    buf[5 * (bb + 16) + 700] ^= 0x08
    with open(path, "wb") as f:
        f.write(buf)
    for d in dev_pages:
        d.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0xBD], {0: ids})
    assert wait_finished(load)[0].success is False
    torch.cuda.synchronize()
    for d in dev_pages:
        assert (d.view(torch.int16) == 0).all(), "a page was written"
    st = eng.stats()
    assert st.checksum_failures == 1
    assert not os.path.exists(path)
    # the key works again
    for d, p in zip(dev_pages, pages):
        d.copy_(p)
    torch.cuda.synchronize()
    store.transfer_async([0xBD], {0: ids})
    assert wait_finished(store)[0].success
    for d in dev_pages:
        d.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0xBD], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    for d, p in zip(dev_pages, pages):
        assert torch.equal(d.cpu()[ids].view(torch.int16),
                           p[ids].view(torch.int16))


def test_gpu_dram_tier_hit_is_verified(tmp_path):
    """Staged path + pinned DRAM tier: the hit (file deleted to prove it) is
    verified on the bounce and loads."""
    shape = SHAPES[0]
    mode, bb, nl, nb = shape
    pages, ids = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(dev_pages, tmp_path, shape, "staged",
                                       host_cache_bytes=8 << 20)
    store.transfer_async([0xCA], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0xCA, 0)
    resident = eng.dram_chunk(path, nb, 0)
    _assert_bytes(resident.numpy(), co.seal(_raw_plain(pages, ids), bb),
                  "DRAM slab")
    os.unlink(path)
    for d in dev_pages:
        d.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0xCA], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    st = eng.stats()
    assert st.host_cache_hits == 1 and st.checksum_failures == 0
    for d, p in zip(dev_pages, pages):
        assert torch.equal(d.cpu()[ids].view(torch.int16),
                           p[ids].view(torch.int16))
