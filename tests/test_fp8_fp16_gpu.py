"""fp16 KV pages through the fp8 HIP kernels on MI355X, byte for byte against
the CPU oracle (fp8_fp16_oracle.py).

The fp16 instantiations of all six kernels (kvc_fp8_amax + kvc_fp8_quant on
the staged per-tile path, kvc_gather_fp8 on the zero-copy one,
kvc_scatter_fp8, kvc_gather_fp8_group<8|16|32|64>, kvc_scatter_fp8_group)
must write and read exactly the oracle's bytes, the same bytes host mode
writes (test_fp8_fp16.py). The inputs carry an fp16-subnormal group/tile
and +-65504 next to zeros and e4m3-exact values, so the f32 -> fp16
rounding on load is checked where it can go wrong: subnormal results must
be kept (not flushed) and rounded to nearest even, and the largest fp16
must come back finite.

The shapes are the ones test_fp8_group_gpu.py and test_fp8_tile_gpu.py
argue for (partly filled waves, single-vector last slices, every group
width, ids through the device id buffer, a second grid-stride trip); the
kernels' control flow does not depend on the page type, so the same
shapes are the smallest at which the fp16 instantiations can go wrong.
"""
import os

import pytest
import torch

import checksum_oracle as co
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

pytestmark = pytest.mark.gpu

# grouped: (block_bytes, group_size, layers, blocks == blocks per file)
G768 = (768, 128, 2, 4)
G8448 = (8448, 128, 2, 4)
G64K = [(65536, g, 4, 16) for g in (64, 128, 256, 512)]
G768_DEV_IDS = (768, 128, 2, 160)
G8448_BIG = (8448, 128, 8, 128)
GROUP_ENGINE = [G768, G8448] + G64K + [G768_DEV_IDS, G8448_BIG]
GROUP_COPIER = [G768, G8448] + G64K + [G8448_BIG]   # copier takes <= 128 ids

# per tile: (block_bytes, None, layers, blocks)
T16 = (16, None, 3, 5)
T1152 = (1152, None, 2, 8)
T8208 = (8208, None, 2, 6)
T768_DEV_IDS = (768, None, 2, 160)
T8448_BIG = (8448, None, 8, 128)
TILE_ENGINE = [T1152, T8208, T768_DEV_IDS, T8448_BIG]
TILE_COPIER = [T16, T1152, T8208, T8448_BIG]


def _id(shape):
    bb, gs, nl, nb = shape
    return f"bb{bb}-" + (f"g{gs}" if gs else "tile") + f"-l{nl}-n{nb}"


def _mode(shape):
    return "fp8_e4m3_group" if shape[1] else "fp8_e4m3"


def _G(shape):
    return shape[1] or shape[0] // 2


_inputs = {}


def cpu_pages(shape):
    """CPU fp16 pages of 2n+2 blocks, the n odd ids the tests move, the
    oracle's record bytes and loaded values; computed once per shape and
    shared read-only."""
    if shape not in _inputs:
        bb, gs, nl, nb = shape
        seed = bb + (gs or 0) + nl + nb
        if gs:
            pages = make_group_pages(2 * nb + 2, bb, gs, nl, seed)
        else:
            pages = make_tile_pages(2 * nb + 2, bb, nl, seed)
        ids = list(range(1, 2 * nb, 2))
        _inputs[shape] = (pages, ids, oracle_records(pages, ids, _G(shape)),
                          loaded_values(pages, ids, _G(shape)))
    return _inputs[shape]


def _engine(pages, tmp, shape, copy_path, **kw):
    bb, gs, nl, nb = shape
    eng = TorchOffloadEngine(
        [pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=nb,
                            copy_path=copy_path, serialize=_mode(shape),
                            fp8_group_size=gs or 128, **kw))
    assert eng.kv_dtype == "float16"
    tag = f"float16+{_mode(shape)}{gs or ''}" + \
        ("+ck" if kw.get("checksum") else "")
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(
        model=f"gf16-{copy_path}", dtype=tag))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [nb]),
            StorageToGPUHandler(eng, mapper, [nb]))


def _assert_bytes(got, want, what):
    assert got.numel() == want.numel(), \
        f"{what}: {got.numel()} bytes, oracle has {want.numel()}"
    diff = (got != want).nonzero().flatten()
    assert diff.numel() == 0, (
        f"{what}: {diff.numel()} of {want.numel()} bytes differ from the "
        f"CPU oracle, first offsets {diff[:8].tolist()}")


def _check_loaded(dev_pages, shape):
    """Moved blocks equal the oracle's values bit for bit (fp16 subnormals
    among them), each group or tile is within 0.07 of its own amax, the
    other blocks stayed zero."""
    bb, gs, nl, nb = shape
    pages, ids, _, deq = cpu_pages(shape)
    others = [i for i in range(2 * nb + 2) if i not in set(ids)]
    subnormal = 0
    for dev, page, y in zip(dev_pages, pages, deq):
        got = dev.cpu()
        bad = (bits(got[ids]) != bits(y)).sum().item()
        sub = count_subnormal(y)
        sub_bad = (bits(got[ids]) != bits(y))[
            (y.float().abs() > 0) & (y.float().abs() < 2.0 ** -14)].sum().item()
        print(f"{bad} of {y.numel()} loaded values differ; "
              f"{sub_bad} of {sub} subnormal ones")
        assert bad == 0
        assert torch.isfinite(got[ids].float()).all()
        assert_group_bound(got[ids], page[ids], _G(shape))
        assert (bits(got[others]) == 0).all()
        subnormal += sub
    assert subnormal > 0, "input exercised no fp16-subnormal result"


def _file_payloads(path, P, checksum):
    raw = open(path, "rb").read()
    if checksum:
        assert co.verify(raw, P) == (0, -1)
        raw = co.payloads(raw, P)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8)


def _roundtrip(tmp_path, shape, copy_path, checksum=False):
    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    eng, mapper, store, load = _engine(dev_pages, tmp_path, shape, copy_path,
                                       checksum=checksum)
    store.transfer_async([0x71], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0x71, 0)
    P = record_bytes(bb, _G(shape))
    assert os.path.getsize(path) == nb * nl * (P + (16 if checksum else 0))
    _assert_bytes(_file_payloads(path, P, checksum), want, "file")
    for t in dev_pages:
        t.zero_()
    torch.cuda.synchronize()
    load.transfer_async([0x71], {0: ids})
    assert wait_finished(load)[0].success
    torch.cuda.synchronize()
    assert eng.stats().errors == 0
    _check_loaded(dev_pages, shape)


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", GROUP_ENGINE + TILE_ENGINE, ids=_id)
def test_gpu_engine_roundtrip_matches_oracle(tmp_path, shape, copy_path):
    _roundtrip(tmp_path, shape, copy_path)


@pytest.mark.parametrize("copy_path", ["staged", "zero_copy"])
@pytest.mark.parametrize("shape", [G8448, T8208], ids=_id)
def test_gpu_engine_roundtrip_with_checksum(tmp_path, shape, copy_path):
    _roundtrip(tmp_path, shape, copy_path, checksum=True)


@pytest.mark.parametrize("shape", GROUP_COPIER + TILE_COPIER, ids=_id)
def test_gpu_block_copier_matches_oracle(shape):
    from llm_d_kv_cache_amd.ops import block_copier

    bb, gs, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    copier = block_copier([dev_pages])
    bf16_copier = block_copier([[p.view(torch.bfloat16) for p in dev_pages]])
    stream = torch.cuda.current_stream().cuda_stream
    if gs:
        nbytes = copier.packed_bytes_fp8_group(0, len(ids), gs)
    else:
        nbytes = copier.packed_bytes_fp8(0, len(ids))
        # the split gather's scratch does not depend on the page type
        assert copier.fp8_scratch_bytes(0, len(ids)) == \
            bf16_copier.fp8_scratch_bytes(0, len(ids))
        scratch = torch.empty(copier.fp8_scratch_bytes(0, len(ids)),
                              dtype=torch.uint8, device="cuda")
    assert nbytes == want.numel()
    # a guard band behind the slab catches a store past the last record
    slab = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    if gs:
        copier.gather_fp8_group(0, ids, slab.data_ptr(), gs, stream)
    else:
        copier.gather_fp8(0, ids, slab.data_ptr(), scratch.data_ptr(), stream)
    torch.cuda.synchronize()
    host = slab.cpu()
    _assert_bytes(host[:nbytes], want, "slab")
    assert (host[nbytes:] == 0xA5).all(), "guard band overwritten"
    for t in dev_pages:
        t.zero_()
    if gs:
        copier.scatter_fp8_group(0, ids, slab.data_ptr(), gs, stream)
    else:
        copier.scatter_fp8(0, ids, slab.data_ptr(), stream)
    torch.cuda.synchronize()
    _check_loaded(dev_pages, shape)


@pytest.mark.parametrize("shape", [G8448, T8208], ids=_id)
def test_files_move_between_gpu_and_host_mode(tmp_path, shape):
    """One file written on the GPU is loaded by a host-mode engine, and one
    host-written file by the GPU engine; both land the oracle's values."""
    bb, gs, nl, nb = shape
    pages, ids, want, deq = cpu_pages(shape)
    dev_pages = [p.cuda() for p in pages]
    host_pages = [p.clone() for p in pages]
    _, gm, gstore, gload = _engine(dev_pages, tmp_path / "gpu", shape,
                                   "staged")
    _, hm, hstore, hload = _engine(host_pages, tmp_path / "host", shape,
                                   "host")
    gstore.transfer_async([0x71], {0: ids})
    hstore.transfer_async([0x71], {0: ids})
    assert wait_finished(gstore)[0].success
    assert wait_finished(hstore)[0].success
    gpath, hpath = gm.file_name(0x71, 0), hm.file_name(0x71, 0)
    gbytes, hbytes = open(gpath, "rb").read(), open(hpath, "rb").read()
    _assert_bytes(torch.frombuffer(bytearray(gbytes), dtype=torch.uint8),
                  want, "GPU file")
    _assert_bytes(torch.frombuffer(bytearray(hbytes), dtype=torch.uint8),
                  want, "host-mode file")
    # swap the files, so each engine loads what the other one wrote
    open(gpath, "wb").write(hbytes)
    open(hpath, "wb").write(gbytes)
    for t in dev_pages + host_pages:
        t.zero_()
    torch.cuda.synchronize()
    gload.transfer_async([0x71], {0: ids})
    hload.transfer_async([0x71], {0: ids})
    assert wait_finished(gload)[0].success
    assert wait_finished(hload)[0].success
    torch.cuda.synchronize()
    _check_loaded(dev_pages, shape)
    for page, y in zip(host_pages, deq):
        assert torch.equal(bits(page[ids]), bits(y))
