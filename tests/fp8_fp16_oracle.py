"""CPU oracle and inputs for both fp8 serialize modes with the page dtype as
a parameter (T = torch.float16 or torch.bfloat16).

Shared by test_fp8_fp16.py (host mode) and test_fp8_fp16_gpu.py (HIP
kernels): both must produce exactly these bytes.

Arithmetic per tile (G = n) or per G-element group, all in f32
(docs/architecture.md):
  amax = max|f32(x)|, 0 -> 1;  scale = amax / 448 (stored);
  inv = 448 / amax;  q = RNE_e4m3fn(f32(x) * inv);
  y = T_RNE(f32(q) * scale).
Both divisions are true f32 divisions, spelled torch.div on two tensors
(see fp8_group_oracle.py for why ``448.0 / amax`` is not one). A record is
T-free: `out_dtype` below is the page type of the LOADING engine, which need
not be the type the record was written from.

For T = fp16 the widening is exact (subnormals included), the load rounds to
nearest even and produces fp16 subnormals, and amax <= 65504 keeps
448 * scale below the 65520 overflow threshold, so y is finite.
"""
import torch

from fp8_group_oracle import (  # noqa: F401  (re-exported for the tests)
    E4M3_MAX,
    REL_BOUND,
    assert_group_bound,
    wait_finished,
)
from fp8_tile_oracle import positions

F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
SUBNORMAL_SCALE = 2.0 ** -17   # randn * this is fp16-subnormal out to 8 sigma

# kinds of special group in make_group_pages
ZERO, EXACT, SUBNORMAL, F16MAX = range(4)


def group_kind(block, layer, group, n_groups):
    """Kind of group `group` of tile (block, layer): 0..3 are the special
    groups above, anything else is plain scaled randn. With five or more
    groups per tile every tile holds all four specials; a shorter tile
    (384 elements = 3 groups) holds n_groups consecutive kinds, rotating
    with block and layer so that any four consecutive blocks cover all."""
    return (group + block + layer) % max(n_groups, 5)


def make_group_pages(num_blocks, block_bytes, group_size, num_layers, seed,
                     dtype=torch.float16):
    """Per-layer pages (num_blocks, block_bytes/2) of `dtype`: randn with
    each group scaled by 10**U(-3, 2), and per tile (see group_kind) an
    all-zero group, a group of exactly representable values (+-448*s,
    0.5*s, s = 2^-3 its scale), a subnormal group (randn * 2^-17) and a
    group holding +-65504."""
    n = block_bytes // 2
    ng = n // group_size
    assert n % group_size == 0
    gen = torch.Generator().manual_seed(seed)
    s = 0.125
    b = torch.arange(num_blocks).view(-1, 1)
    g = torch.arange(ng).view(1, -1)
    pages = []
    for layer in range(num_layers):
        x = torch.randn(num_blocks, ng, group_size, generator=gen)
        x *= 10.0 ** (torch.rand(num_blocks, ng, 1, generator=gen) * 5 - 3)
        kind = group_kind(b, layer, g, ng)
        x[kind == ZERO] = 0.0
        ex = torch.randn(num_blocks, ng, group_size, generator=gen) * s
        ex[..., 0] = E4M3_MAX * s
        ex[..., 1] = -E4M3_MAX * s
        ex[..., 2] = 0.5 * s
        x[kind == EXACT] = ex[kind == EXACT]
        sub = torch.randn(num_blocks, ng, group_size,
                          generator=gen) * SUBNORMAL_SCALE
        x[kind == SUBNORMAL] = sub[kind == SUBNORMAL]
        big = torch.randn(num_blocks, ng, group_size, generator=gen) * 1000.0
        big[..., 0] = F16_MAX
        big[..., group_size - 1] = -F16_MAX
        x[kind == F16MAX] = big[kind == F16MAX]
        pages.append(x.reshape(num_blocks, n).to(dtype))
    return pages


def make_tile_pages(num_blocks, block_bytes, num_layers, seed,
                    dtype=torch.float16):
    """Per-layer pages (num_blocks, block_bytes/2) of `dtype`, finite only.

    As fp8_tile_oracle.make_tile_pages: randn clamped to +-3 times a
    per-tile 10**U(-3, 2), one planted maximum of +-4 * max|tile| at
    positions(n)[t % 8]. Block 1 is all zeros, block 3 all fp16-subnormal
    (randn * 2^-17, planted maximum included) and block 5 has +-65504 as its
    planted maximum, with -+65504 in the element after it (odd blocks: the
    tests move those)."""
    n = block_bytes // 2
    pos = positions(n)
    gen = torch.Generator().manual_seed(seed)
    blocks = torch.arange(num_blocks)
    pages = []
    for layer in range(num_layers):
        x = torch.randn(num_blocks, n, generator=gen).clamp_(-3.0, 3.0)
        x *= 10.0 ** (torch.rand(num_blocks, 1, generator=gen) * 5 - 3)
        if num_blocks > 3:
            x[3] = torch.randn(n, generator=gen).clamp_(-3.0, 3.0) \
                * SUBNORMAL_SCALE
        t = blocks * num_layers + layer
        where = torch.tensor(pos)[t % 8]
        sign = 1.0 - 2.0 * (t % 2).float()
        peak = 4.0 * x.abs().amax(1).clamp_min(1e-30)
        if num_blocks > 5:
            peak[5] = F16_MAX
        x[blocks, where] = sign * peak
        if num_blocks > 5:
            x[5, (where[5] + 1) % n] = -sign[5] * F16_MAX
        if num_blocks > 1:
            x[1] = 0.0
        pages.append(x.to(dtype))
    return pages


def oracle(x, group_size, out_dtype=None):
    """x: fp16 or bf16 (..., n). Returns (q uint8 (..., n), scales f32
    (..., n/G), y out_dtype (..., n), amax f32 (..., n/G)); out_dtype
    defaults to x's own dtype."""
    out_dtype = out_dtype or x.dtype
    lead, n = x.shape[:-1], x.shape[-1]
    xg = x.float().reshape(*lead, n // group_size, group_size)
    amax = xg.abs().amax(-1, keepdim=True)
    amax = torch.where(amax == 0, torch.ones_like(amax), amax)
    inv = torch.div(torch.full_like(amax, E4M3_MAX), amax)
    scale = torch.div(amax, torch.full_like(amax, E4M3_MAX))
    q = (xg * inv).to(torch.float8_e4m3fn)
    y = (q.float() * scale).to(out_dtype)
    return (q.view(torch.uint8).reshape(*lead, n),
            scale.reshape(*lead, n // group_size),
            y.reshape(*lead, n),
            amax.reshape(*lead, n // group_size))


def oracle_records(pages, ids, group_size):
    """Expected file/slab bytes for blocks `ids`: records
    [n fp8 | n/G f32 scales], block-major, layer-minor. uint8 1-D.
    group_size = n gives the per-tile records."""
    recs = []
    for page in pages:
        q, scale, _, _ = oracle(page[ids].cpu(), group_size)
        recs.append(torch.cat(
            [q, scale.contiguous().view(torch.uint8).reshape(len(ids), -1)],
            dim=1))
    return torch.stack(recs, dim=1).reshape(-1)


def loaded_values(pages, ids, group_size, out_dtype=None):
    """Per layer, the values a load of `ids` must produce."""
    return [oracle(p[ids].cpu(), group_size, out_dtype)[2] for p in pages]


def record_bytes(block_bytes, group_size):
    n = block_bytes // 2
    return n + 4 * (n // group_size)


def bits(t):
    """16-bit pages of any dtype (or uint8 views of them) as int16."""
    return t.contiguous().view(torch.int16)


def count_subnormal(y):
    """Nonzero fp16-subnormal values in y (fp16)."""
    a = y.float().abs()
    return int(((a > 0) & (a < F16_MIN_NORMAL)).sum())
