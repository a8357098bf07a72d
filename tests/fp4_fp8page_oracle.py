"""CPU oracle and inputs for serialize="fp4_e2m1_group" over fp8 (OCP
e4m3fn) pages, kv_dtype="float8_e4m3fn".

Shared by test_fp4_fp8page.py (host mode) and test_fp4_fp8page_gpu.py (HIP
kernels): both must produce exactly these bytes.

Arithmetic per G-element group, all in f32 (docs/architecture.md); a tile of
block_bytes holds n = block_bytes elements:
  x = exact f32 value of the page byte;  amax = max|x|, 0 -> 1;
  scale = amax / 6 (stored);  inv = 6 / amax;  t = x * inv;
  code = signbit(x) << 3 | mag(|t|), mag the e2m1 compare chain of
  fp4_group_oracle.encode;
  load: p = f32(value(code)) * scale, y = RNE_e4m3fn(p): ties to even,
  subnormals kept, the sign copied onto a zero magnitude (-0.0 and negatives
  that underflow give 0x80).

Pages are moved around as uint8 here; the page -> f32 conversion is
``.view(torch.float8_e4m3fn).float()`` and the final rounding is
``.to(torch.float8_e4m3fn)``. Both divisions are torch.div on two tensors
(see fp4_group_oracle.py for why).

Record: [ n/2 code bytes | n/G f32 scales ], element 2i in bits 3:0 of byte
i. NaN page bytes (0x7f, 0xff) are out of scope and appear nowhere below.
"""
import torch

from fp4_group_oracle import (  # noqa: F401  (re-exported for the tests)
    MAGNITUDES,
    all_codes_slab,
    assert_bytes,
    encode,
    pack_codes,
    unpack_codes,
    wait_finished,
)

E2M1_MAX = 6.0
E4M3_MAX = 448.0
GROUP_SIZES = (16, 32, 64, 128)
F8 = torch.float8_e4m3fn

# the exact group's first 16 elements and their codes: amax 48 = 6 * 8, so
# inv = 1/8 is exact and the elements sit on every e2m1 value and tie. All
# of them are e4m3 values; -2^-9 (the smallest subnormal) encodes to -0 and
# loads as 0x80, like the -0.0 next to it.
EXACT_VALUES = (48.0, -48.0, 2.0, 6.0, 10.0, 14.0, 20.0, 28.0, 40.0, -2.0,
                -10.0, -20.0, -40.0, -0.0, -2.0 ** -9, 4.0)
EXACT_CODES = (0x7, 0xF, 0x0, 0x2, 0x2, 0x4, 0x4, 0x6, 0x6, 0x8, 0xA, 0xC,
               0xE, 0x8, 0x8, 0x1)
EXACT_SCALE = 8.0


def to_f32(u8):
    """uint8 page bytes -> their exact f32 values."""
    return u8.contiguous().view(F8).float()


def from_f32(p):
    """f32 -> e4m3fn bytes (uint8): the load's final rounding."""
    return p.to(F8).view(torch.uint8)


def as_u8(t):
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def finite_bytes():
    """The 254 finite e4m3fn bytes."""
    b = torch.arange(256, dtype=torch.int64)
    return b[(b & 0x7f) != 0x7f].to(torch.uint8)


def amax_bytes():
    """The 126 positive finite e4m3fn bytes: every amax a group can have."""
    return torch.arange(1, 0x7f, dtype=torch.int64).to(torch.uint8)


def decode(codes, scale):
    """codes uint8 (..., G) of 4-bit codes, scale f32 (..., 1) -> page bytes
    (uint8): the f32 product, then one rounding to e4m3fn."""
    lut = torch.tensor(MAGNITUDES, dtype=torch.float32)
    val = lut[(codes & 7).long()]
    val = torch.where((codes & 8) != 0, -val, val)
    return from_f32(val * scale)


def oracle(x, group_size):
    """x: uint8 or float8_e4m3fn (..., n). Returns (codes uint8 (..., n), one
    4-bit code per element, scales f32 (..., n/G), y uint8 (..., n), amax
    f32 (..., n/G))."""
    x = as_u8(x)
    lead, n = x.shape[:-1], x.shape[-1]
    xg = to_f32(x).reshape(*lead, n // group_size, group_size)
    amax = xg.abs().amax(-1, keepdim=True)
    amax = torch.where(amax == 0, torch.ones_like(amax), amax)
    inv = torch.div(torch.full_like(amax, E2M1_MAX), amax)
    scale = torch.div(amax, torch.full_like(amax, E2M1_MAX))
    codes = encode(xg * inv) | (torch.signbit(xg).to(torch.uint8) << 3)
    y = decode(codes, scale)
    return (codes.reshape(*lead, n),
            scale.reshape(*lead, n // group_size),
            y.reshape(*lead, n),
            amax.reshape(*lead, n // group_size))


def _exhaustive_rel_bound():
    """max |y - x| / amax over all 126 amax values x 254 finite x with
    |x| <= amax, each pair as the group [amax, x] (a group's other members
    do not enter x's code or y). The ratio is a float64 division of exact
    float64 differences, the same expression assert_group_bound uses."""
    a = to_f32(amax_bytes())[:, None]                     # (126, 1)
    x = to_f32(finite_bytes())[None, :]                   # (1, 254)
    inv = torch.div(torch.full_like(a, E2M1_MAX), a)
    scale = torch.div(a, torch.full_like(a, E2M1_MAX))
    codes = encode(x * inv) | (torch.signbit(x).to(torch.uint8) << 3)
    y = to_f32(decode(codes, scale))
    p = torch.tensor(MAGNITUDES)[(codes & 7).long()] * scale
    assert (p.abs() <= E4M3_MAX).all()          # no load reaches the NaN code
    ok = x.abs() <= a
    assert (y.abs() <= a)[ok].all()
    rel = (y.double() - x.double()).abs() / a.double()
    return rel[ok].max().item()


# |y - x| <= REL_BOUND * group amax: the exhaustive maximum, recomputed here,
# not a tuned number. It is attained at amax = 5 * 2^-9, x = 4 * 2^-9
# (t = 4.8 -> 4, p = 3.33 * 2^-9 -> 3 * 2^-9).
REL_BOUND = _exhaustive_rel_bound()
assert 0.19 < REL_BOUND <= 0.2 + 1e-6, REL_BOUND


def record_bytes(block_bytes, group_size):
    return block_bytes // 2 + 4 * block_bytes // group_size


def group_kind(block, j, ng):
    """What make_pages puts into group j of tile `block` (every layer):
    "zero", "sub" (subnormals only), "exact" or "random"."""
    return {0: "zero", 1: "sub", 3: "exact"}.get((block * ng + j) % 5,
                                                 "random")


def max_position(block, j, ng, group_size):
    """Where make_pages plants the maximum of a "random" or "sub" group:
    byte 0 of its first lane, byte 15 of its first lane, byte 0 of its last
    lane, its last byte, in turn (a lane holds 16 page bytes)."""
    return (0, 15, group_size - 16, group_size - 1)[(block * ng + j) % 4]


def make_pages(num_blocks, block_bytes, group_size, num_layers, seed):
    """Per-layer float8_e4m3fn pages (num_blocks, block_bytes). Group j of
    tile b is, by group_kind(b, j, ng): all zero; subnormals only; the exact
    group (EXACT_VALUES first, the rest within +-40); or random values whose
    per-group magnitude is spread over the whole e4m3 range, 2^-9 .. 448.
    Random and subnormal groups hold ONE strict maximum, planted at
    max_position(b, j, ng, G): a butterfly or a 16-value lane maximum that
    drops an element gets that group's scale wrong."""
    n = block_bytes
    G = group_size
    ng = n // G
    assert n % G == 0 and ng >= 1
    gen = torch.Generator().manual_seed(seed)
    planted = torch.tensor(EXACT_VALUES, dtype=torch.float32)
    step = 2.0 ** -9
    f = torch.arange(num_blocks * ng)
    zero, sub, exact = f % 5 == 0, f % 5 == 1, f % 5 == 3
    rand = ~(zero | sub | exact)
    pos = torch.tensor([0, 15, G - 16, G - 1])[f % 4]
    pages = []
    for _ in range(num_layers):
        x = torch.randn(num_blocks * ng, G, generator=gen)
        x *= 2.0 ** (torch.rand(num_blocks * ng, 1, generator=gen) * 16 - 9)
        # round to e4m3 now, below the largest value, so that 1.5 x the
        # group's maximum is still finite and strictly larger after rounding
        x = to_f32(from_f32(x.clamp(-256.0, 256.0)))
        sign = torch.where(torch.rand(num_blocks * ng, generator=gen) < 0.5,
                           -1.0, 1.0)
        x[zero] = 0.0
        x[sub] = torch.randint(-6, 7, (int(sub.sum()), G),
                               generator=gen).float() * step
        x[exact] = to_f32(from_f32(
            (torch.randn(int(exact.sum()), G, generator=gen) * 8.0)
            .clamp(-40.0, 40.0)))
        x[exact, :16] = planted
        top = to_f32(from_f32((x.abs().amax(1) * 1.5).clamp(step, E4M3_MAX)))
        top[sub] = 7 * step
        rows = (sub | rand).nonzero().flatten()
        x[rows, pos[rows]] = (sign * top)[rows]
        assert (x[rows].abs() == top[rows, None]).sum(1).eq(1).all()
        page = from_f32(x.reshape(num_blocks, n))
        assert ((page & 0x7f) != 0x7f).all()
        pages.append(page.view(F8))
    return pages


def oracle_records(pages, ids, group_size):
    """Expected file/slab bytes for blocks `ids`: records
    [n/2 code bytes | n/G f32 scales], block-major, layer-minor. uint8
    1-D."""
    recs = []
    for page in pages:
        codes, scale, _, _ = oracle(as_u8(page.cpu())[ids], group_size)
        recs.append(torch.cat(
            [pack_codes(codes),
             scale.contiguous().view(torch.uint8).reshape(len(ids), -1)],
            dim=1))
    return torch.stack(recs, dim=1).reshape(-1)


def assert_group_bound(got, want, group_size):
    """Every group: max|got - want| <= REL_BOUND * that group's amax."""
    got, want = as_u8(got), as_u8(want)
    lead, n = want.shape[:-1], want.shape[-1]
    w = to_f32(want).double().reshape(*lead, n // group_size, group_size)
    g = to_f32(got).double().reshape(*lead, n // group_size, group_size)
    err = (g - w).abs().amax(-1)
    amax = w.abs().amax(-1)
    assert (err[amax == 0] == 0).all()
    rel = (err / amax.clamp_min(2.0 ** -9)).max().item()
    print(f"per-group max err/amax = {rel:.4f} (bound {REL_BOUND:.4f})")
    assert rel <= REL_BOUND, f"group error {rel} * amax exceeds {REL_BOUND}"


def assert_page_bits(got, want, what):
    """Byte-for-byte equality of two fp8 page tensors (0x80 != 0x00)."""
    got, want = as_u8(got), as_u8(want)
    assert got.shape == want.shape
    diff = (got != want).nonzero()
    assert diff.numel() == 0, (
        f"{what}: {diff.shape[0]} page bytes differ from the CPU oracle, "
        f"first at {diff[:4].tolist()}")


# ---- every (amax, x) pair as a G=16 group -----------------------------------

EXHAUSTIVE_TILE_BYTES = 1024  # 64 groups of 16
_exhaustive = {}


def exhaustive_page():
    """uint8 (blocks, 1024): for each of the 126 amax values, with either
    sign, G=16 groups [amax, 15 x] that run through every finite x with
    |x| <= amax (both zeros included), zero padded; about 2200 groups."""
    if "page" not in _exhaustive:
        fin = finite_bytes()
        mag = to_f32(fin).abs()
        groups = []
        for a in amax_bytes().tolist():
            xs = fin[mag <= to_f32(torch.tensor([a], dtype=torch.uint8))[0]]
            pad = (-xs.numel()) % 15
            xs = torch.cat([xs, torch.zeros(pad, dtype=torch.uint8)])
            xs = xs.reshape(-1, 15)
            for head in (a, a | 0x80):
                col = torch.full((xs.shape[0], 1), head, dtype=torch.uint8)
                groups.append(torch.cat([col, xs], dim=1))
        flat = torch.cat(groups).reshape(-1)
        blocks = -(-flat.numel() // EXHAUSTIVE_TILE_BYTES)
        page = torch.zeros(blocks, EXHAUSTIVE_TILE_BYTES, dtype=torch.uint8)
        page.view(-1)[:flat.numel()] = flat
        assert 2000 * 16 <= flat.numel() <= 40 * 1024
        _exhaustive["page"] = page
    return _exhaustive["page"]


def decode_scales():
    """The 126 scales amax / 6 our encoders can write for nonzero groups."""
    a = to_f32(amax_bytes())
    return torch.div(a, torch.full_like(a, E2M1_MAX))
