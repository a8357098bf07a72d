"""serialize="fp8_e4m3" (one f32 scale per tile) on the host path, held to
the torch oracle in fp8_tile_oracle.py byte for byte.

The HIP kernels are held to the same bytes in test_fp8_tile_gpu.py, so a
host-mode engine and a GPU engine write the same file for the same KV
blocks. That needs the software encoder to round exact ties to even, as
v_cvt_pk_fp8_f32 and the oracle do: a tile whose amax has mantissa 1.75
gets a power-of-two scale, every bf16 value then scales exactly, and about
0.4 % of them land on a tie.
"""
import os

import pytest
import torch

import checksum_oracle as co
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

# (block_bytes, num_layers, blocks == blocks per file): one 16-byte vector
# per tile with a 12-byte record; 576 elements; 4104 elements, where the
# last planted maximum sits in the kernels' third slice
SHAPES = [(16, 3, 5), (1152, 2, 8), (8208, 2, 6)]
SHAPE_IDS = [f"bb{b}-l{l}-n{n}" for b, l, n in SHAPES]

_inputs = {}


def cpu_pages(shape):
    """Pages of 2n+2 blocks, the n odd ids the tests move, the oracle's
    record bytes and dequantized values; computed once, shared read-only."""
    if shape not in _inputs:
        bb, nl, nb = shape
        pages = make_tile_pages(2 * nb + 2, bb, nl, seed=bb + nl + nb)
        ids = list(range(1, 2 * nb, 2))
        _inputs[shape] = (pages, ids, tile_records(pages, ids),
                          tile_values(pages, ids))
    return _inputs[shape]


def _assert_bytes(got, want, what):
    assert got.numel() == want.numel(), \
        f"{what}: {got.numel()} bytes, oracle has {want.numel()}"
    diff = (got != want).nonzero().flatten()
    assert diff.numel() == 0, (
        f"{what}: {diff.numel()} of {want.numel()} bytes differ from the "
        f"oracle, first offsets {diff[:8].tolist()}")


def _check_loaded(pages_now, shape):
    bb, nl, nb = shape
    pages, ids, _, deq = cpu_pages(shape)
    others = [i for i in range(2 * nb + 2) if i not in set(ids)]
    for got, page, y in zip(pages_now, pages, deq):
        assert torch.equal(got[ids].view(torch.int16), y.view(torch.int16))
        assert_tile_bound(got[ids], page[ids])
        assert (got[others].view(torch.int16) == 0).all()


def test_input_has_its_planted_shape():
    """The oracle sees what make_tile_pages promises: block 1 is zero with
    scale 1/448, every other tile's amax is the planted value, and
    neighbouring tiles' scales are far apart somewhere."""
    pages, ids, _, _ = cpu_pages(SHAPES[2])
    nl, n = len(pages), pages[0].shape[1]
    from fp8_tile_oracle import positions

    pos = positions(n)
    for layer, page in enumerate(pages):
        q, scale, _, amax = tile_oracle(page)
        assert (q[1] == 0).all()
        assert scale[1].item() == torch.div(torch.tensor(1.0),
                                            torch.tensor(448.0)).item()
        for b in range(page.shape[0]):
            if b == 1:
                continue
            t = b * nl + layer
            peak = page[b, pos[t % 8]].float()
            assert peak.abs().item() == amax[b].item()
            assert (peak > 0) == (t % 2 == 0)
            rest = page[b].float().abs()
            rest[pos[t % 8]] = 0
            assert rest.max().item() <= 0.26 * amax[b].item()
        ratio = scale[1:].flatten() / scale[:-1].flatten()
        assert ratio.max() > 100 or ratio.min() < 0.01


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_block_copier_host_matches_oracle(shape):
    from llm_d_kv_cache_amd.ops import block_copier

    bb, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    work = [p.clone() for p in pages]
    copier = block_copier([work])
    nbytes = copier.packed_bytes_fp8(0, len(ids))
    assert nbytes == nb * nl * record_bytes(bb) == want.numel()
    slab = torch.full((nbytes,), 0xA5, dtype=torch.uint8)
    copier.gather_fp8(0, ids, slab.data_ptr(), 0, 0)
    _assert_bytes(slab, want, "slab")
    # scatter the ORACLE's bytes, so the decoder is checked on its own
    for p in work:
        p.zero_()
    src = want.clone()
    copier.scatter_fp8(0, ids, src.data_ptr(), 0)
    _check_loaded(work, shape)


def _engine(pages, tmp, shape, checksum=False):
    bb, nl, nb = shape
    eng = TorchOffloadEngine(
        [pages],
        OffloadEngineConfig(io_threads=2, gpu_blocks_per_file=nb,
                            copy_path="host", serialize="fp8_e4m3",
                            checksum=checksum))
    mapper = FileMapper(str(tmp), KVCacheLayoutConfig(
        model="fp8t", dtype="bfloat16+fp8_e4m3" + ("+ck" if checksum else "")))
    return (eng, mapper, GPUToStorageHandler(eng, mapper, [nb]),
            StorageToGPUHandler(eng, mapper, [nb]))


@pytest.mark.parametrize(
    "shape,checksum",
    [(s, False) for s in SHAPES] + [(SHAPES[1], True)],
    ids=SHAPE_IDS + [SHAPE_IDS[1] + "-ck"])
def test_engine_host_matches_oracle(tmp_path, shape, checksum):
    """A host-mode store writes the oracle's file and loads the oracle's
    values; with checksum=True the payloads are the same bytes and every
    footer verifies."""
    bb, nl, nb = shape
    pages, ids, want, _ = cpu_pages(shape)
    work = [p.clone() for p in pages]
    eng, mapper, store, load = _engine(work, tmp_path, shape, checksum)
    store.transfer_async([0x71], {0: ids})
    assert wait_finished(store)[0].success
    path = mapper.file_name(0x71, 0)
    raw = open(path, "rb").read()
    P = record_bytes(bb)
    assert os.path.getsize(path) == nb * nl * (P + (16 if checksum else 0))
    if checksum:
        assert co.verify(raw, P) == (0, -1)
        raw = co.payloads(raw, P)
    _assert_bytes(torch.frombuffer(bytearray(raw), dtype=torch.uint8), want,
                  "file")
    for p in work:
        p.zero_()
    load.transfer_async([0x71], {0: ids})
    assert wait_finished(load)[0].success
    assert eng.stats().errors == 0
    _check_loaded(work, shape)


def _host_roundtrip(page):
    """One (1, n) bf16 tile through BlockCopier's CPU path: (record bytes,
    round-tripped tile)."""
    from llm_d_kv_cache_amd.ops import block_copier

    work = page.clone()
    copier = block_copier([[work]])
    slab = torch.zeros(copier.packed_bytes_fp8(0, 1), dtype=torch.uint8)
    copier.gather_fp8(0, [0], slab.data_ptr(), 0, 0)
    work.zero_()
    copier.scatter_fp8(0, [0], slab.data_ptr(), 0)
    return slab, work


def test_negative_zero_keeps_its_sign():
    """Every third value -0.0: encoded 0x80 like the oracle, never 0x00."""
    n = 576
    page = make_tile_pages(2, 2 * n, 1, seed=9)[0][:1].clone()
    page[0, ::3] = -0.0
    slab, back = _host_roundtrip(page)
    assert (slab[:n][::3] == 0x80).all()
    _assert_bytes(slab, tile_records([page], [0]), "slab")
    assert torch.equal(back.view(torch.int16),
                       tile_oracle(page)[2].view(torch.int16))
    assert (back[0, ::3].view(torch.int16) == -0x8000).all()


def test_nan_element_stays_nan_and_leaves_the_tile_alone():
    """One NaN in a tile: that element is stored as 0x7f and loads as NaN;
    it does not enter the amax, so every other element equals the oracle of
    the same tile with the NaN replaced by 0."""
    n, at = 576, 100
    page = make_tile_pages(2, 2 * n, 1, seed=10)[0][:1].clone()
    clean = page.clone()
    clean[0, at] = 0.0
    page[0, at] = float("nan")
    slab, back = _host_roundtrip(page)
    want = tile_records([clean], [0])
    assert slab[at].item() == 0x7F
    keep = torch.ones(n + 4, dtype=torch.bool)
    keep[at] = False
    _assert_bytes(slab[keep], want[keep], "slab without the NaN byte")
    y = tile_oracle(clean)[2]
    assert torch.isnan(back[0, at])
    assert torch.equal(back[0, keep[:n]].view(torch.int16),
                       y[0, keep[:n]].view(torch.int16))
