"""CPU oracle and planted-maximum input for serialize="fp8_e4m3" (one f32
scale per (block, layer) tile).

The per-tile arithmetic is the group arithmetic of fp8_group_oracle.py with
G = n, the whole tile, so the oracle is that module's with group_size = n.
Shared by test_fp8_tile.py (host mode) and test_fp8_tile_gpu.py (HIP
kernels): both must produce exactly these bytes.

Arithmetic per tile of n bf16 values, all in f32 (docs/architecture.md):
  amax = max|x|, 0 -> 1;  scale = amax / 448 (stored);  inv = 448 / amax;
  q = RNE_e4m3fn(x * inv);  y = bf16_RNE(f32(q) * scale).

`inv` is a true f32 division (torch.div on two tensors inside
fp8_group_oracle.oracle). ``448.0 / amax`` on a tensor is NOT that: it
evaluates ``amax.reciprocal() * 448.0``, two roundings, and differs from the
division in the last bit for about a quarter of all amax values.
"""
import torch

from fp8_group_oracle import (  # noqa: F401  (re-exported for the tests)
    REL_BOUND,
    assert_group_bound,
    oracle,
    oracle_records,
    wait_finished,
)


def positions(n):
    """Where make_tile_pages plants the tile maximum, by tile index mod 8:
    the low and high halves of the first dword, the end of the first 16-byte
    vector, lane 63 of wave 0, lane 0 of wave 1, the last lane of workgroup
    slice 0, the first lane of slice 1, and the last element (each taken
    mod n for tiles shorter than that)."""
    return [p % n for p in
            (0, 1, 7, 8 * 63 + 7, 8 * 64, 8 * 255 + 7, 8 * 256, n - 1)]


def make_tile_pages(num_blocks, block_bytes, num_layers, seed):
    """Per-layer bf16 pages (num_blocks, block_bytes/2), finite values only.

    Tile t = block * num_layers + layer holds randn clamped to +-3 times
    10**U(-3, 2) drawn per tile — so a scale taken from a neighbouring tile
    is off by orders of magnitude — and one planted maximum of
    +-4 * max|tile| at positions(n)[t % 8], its sign alternating with t. The
    clamp makes the planted value the tile's amax whatever randn drew, so a
    reduction that loses the lane, wave or slice holding it gets the scale,
    and with it nearly every byte, wrong. Block 1 of every layer is all
    zeros (scale 1/448, payload 0x00)."""
    n = block_bytes // 2
    pos = positions(n)
    gen = torch.Generator().manual_seed(seed)
    blocks = torch.arange(num_blocks)
    pages = []
    for layer in range(num_layers):
        x = torch.randn(num_blocks, n, generator=gen).clamp_(-3.0, 3.0)
        x *= 10.0 ** (torch.rand(num_blocks, 1, generator=gen) * 5 - 3)
        t = blocks * num_layers + layer
        where = torch.tensor(pos)[t % 8]
        sign = 1.0 - 2.0 * (t % 2).float()
        peak = 4.0 * x.abs().amax(1).clamp_min(1e-30)
        x[blocks, where] = sign * peak
        if num_blocks > 1:
            x[1] = 0.0
        pages.append(x.to(torch.bfloat16))
    return pages


def tile_oracle(x):
    """x: bf16 (..., n), one tile per row. Returns (q uint8 (..., n),
    scale f32 (..., 1), y bf16 (..., n), amax f32 (..., 1))."""
    return oracle(x, x.shape[-1])


def tile_records(pages, ids):
    """Expected file/slab bytes for blocks `ids`: records [n fp8 | f32
    scale], block-major, layer-minor. uint8 1-D."""
    return oracle_records(pages, ids, pages[0].shape[-1])


def tile_values(pages, ids):
    """Per layer, the dequantized bf16 values a load of `ids` must produce."""
    return [tile_oracle(p[ids])[2] for p in pages]


def record_bytes(block_bytes):
    return block_bytes // 2 + 4


def assert_tile_bound(got, want):
    """Every tile: max|got - want| <= REL_BOUND * that tile's amax."""
    assert_group_bound(got, want, want.shape[-1])
