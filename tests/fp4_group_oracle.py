"""CPU oracle and inputs for serialize="fp4_e2m1_group".

Shared by test_fp4_group.py (host mode) and test_fp4_group_gpu.py (HIP
kernels): both must produce exactly these bytes, which is what lets files
move between GPU and host-mode engines.

Arithmetic per G-element group, all in f32 (docs/architecture.md):
  amax = max|x|, 0 -> 1;  scale = amax / 6 (stored);  inv = 6 / amax;
  t = x * inv;  code = signbit(x) << 3 | mag(|t|), mag = round-to-nearest-
  even on the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6}, saturating;
  y = T_RNE(f32(value(code)) * scale), T the page type (two roundings).

Both divisions are true f32 divisions, spelled torch.div on two tensors.
The Python expression ``6.0 / amax`` on a tensor is NOT that:
Tensor.__rtruediv__ evaluates ``amax.reciprocal() * 6.0``, two roundings,
which differs from the division in the last bit for many amax values (see
fp8_group_oracle.py).

Record: [ n/2 code bytes | n/G f32 scales ], n = block_bytes/2; element 2i
in bits 3:0 of byte i, element 2i+1 in bits 7:4.
"""
import time

import numpy as np
import torch

E2M1_MAX = 6.0
MAGNITUDES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
GROUP_SIZES = (16, 32, 64, 128)
# |y - x| <= REL_BOUND * group_amax, derived, not tuned: t = x * inv lies in
# [-6, 6], where the widest e2m1 gap (4 to 6) is 2, so rounding to nearest
# moves t by at most 1, i.e. amax/6 = 0.1667 amax; page rounding of y adds
# at most 2^-9 |y| <= 0.002 amax (bf16; fp16 less), the f32 roundings ~2^-23.
REL_BOUND = 0.17

# the exact group's first 16 elements in units of s, and their codes
EXACT_UNITS = (6.0, -6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25,
               -1.25, -2.5, -5.0, -0.0, -2.0 ** -20, 0.5)
EXACT_CODES = (0x7, 0xF, 0x0, 0x2, 0x2, 0x4, 0x4, 0x6, 0x6, 0x8, 0xA, 0xC,
               0xE, 0x8, 0x8, 0x1)
EXACT_S = 0.125

# fp16 tie page: one G=16 group per tie amax, padded to this tile
TIE_TILE_BYTES = 22528


def make_pages(num_blocks, block_bytes, group_size, num_layers, seed,
               dtype=torch.bfloat16):
    """Per-layer pages (num_blocks, block_bytes/2): randn with each group
    scaled by 10**U(-3, 2), plus in every tile one all-zero group and one
    exact group: amax 6s with s = 2^-3, so inv = 1/s is exact and its first
    16 elements (EXACT_UNITS * s) sit on every e2m1 value and tie."""
    n = block_bytes // 2
    ng = n // group_size
    assert n % group_size == 0 and ng >= 2
    gen = torch.Generator().manual_seed(seed)
    s = EXACT_S
    planted = torch.tensor(EXACT_UNITS, dtype=torch.float32) * s
    pages = []
    for _ in range(num_layers):
        x = torch.randn(num_blocks, ng, group_size, generator=gen)
        x *= 10.0 ** (torch.rand(num_blocks, ng, 1, generator=gen) * 5 - 3)
        blocks = torch.arange(num_blocks)
        x[blocks, blocks % ng] = 0.0               # an all-zero group
        exact = (blocks + 1) % ng                  # a different group
        x[blocks, exact] = (torch.randn(num_blocks, group_size,
                                        generator=gen) * s).clamp(-5 * s, 5 * s)
        x[blocks, exact, :16] = planted
        pages.append(x.reshape(num_blocks, n).to(dtype))
    return pages


def encode(t):
    """t f32 -> e2m1 magnitude code 0..7 (uint8): RNE, ties to the even
    code, saturating."""
    a = t.abs()
    mag = torch.zeros_like(a, dtype=torch.uint8)
    for thr, inclusive in ((0.25, False), (0.75, True), (1.25, False),
                           (1.75, True), (2.5, False), (3.5, True),
                           (5.0, False)):
        mag += (a >= thr if inclusive else a > thr).to(torch.uint8)
    return mag


def decode(codes, scale, dtype):
    """codes uint8 (..., G) of 4-bit codes, scale f32 (..., 1) -> page
    values: the f32 product, then one rounding to dtype."""
    lut = torch.tensor(MAGNITUDES, dtype=torch.float32)
    val = lut[(codes & 7).long()]
    val = torch.where((codes & 8) != 0, -val, val)
    return (val * scale).to(dtype)


def oracle(x, group_size):
    """x: bf16 or fp16 (..., n). Returns (codes uint8 (..., n), one 4-bit
    code per element, scales f32 (..., n/G), y like x, amax f32
    (..., n/G))."""
    lead, n = x.shape[:-1], x.shape[-1]
    xg = x.float().reshape(*lead, n // group_size, group_size)
    amax = xg.abs().amax(-1, keepdim=True)
    amax = torch.where(amax == 0, torch.ones_like(amax), amax)
    inv = torch.div(torch.full_like(amax, E2M1_MAX), amax)
    scale = torch.div(amax, torch.full_like(amax, E2M1_MAX))
    codes = encode(xg * inv) | (torch.signbit(xg).to(torch.uint8) << 3)
    y = decode(codes, scale, x.dtype)
    return (codes.reshape(*lead, n),
            scale.reshape(*lead, n // group_size),
            y.reshape(*lead, n),
            amax.reshape(*lead, n // group_size))


def pack_codes(codes):
    """(..., n) 4-bit codes -> (..., n/2) bytes, even element low."""
    return codes[..., 0::2] | (codes[..., 1::2] << 4)


def unpack_codes(packed):
    """(..., m) bytes -> (..., 2m) 4-bit codes."""
    return torch.stack([packed & 0xf, packed >> 4], dim=-1).flatten(-2)


def oracle_records(pages, ids, group_size):
    """Expected file/slab bytes for blocks `ids`: records
    [n/2 code bytes | n/G f32 scales], block-major, layer-minor. uint8
    1-D."""
    recs = []
    for page in pages:
        codes, scale, _, _ = oracle(page[ids].cpu(), group_size)
        recs.append(torch.cat(
            [pack_codes(codes),
             scale.contiguous().view(torch.uint8).reshape(len(ids), -1)],
            dim=1))
    return torch.stack(recs, dim=1).reshape(-1)


def record_bytes(block_bytes, group_size):
    n = block_bytes // 2
    return n // 2 + 4 * n // group_size


def assert_group_bound(got, want, group_size):
    """Every group: max|got - want| <= REL_BOUND * that group's amax."""
    lead, n = want.shape[:-1], want.shape[-1]
    w = want.float().reshape(*lead, n // group_size, group_size)
    g = got.float().reshape(*lead, n // group_size, group_size)
    err = (g - w).abs().amax(-1)
    amax = w.abs().amax(-1)
    worst = (err - REL_BOUND * amax).max().item()
    rel = (err / amax.clamp_min(1e-30)).max().item()
    print(f"per-group max err/amax = {rel:.4f} (bound {REL_BOUND})")
    assert worst <= 0, f"group error exceeds {REL_BOUND} * amax (rel {rel})"


def assert_bytes(got, want, what):
    assert got.numel() == want.numel(), \
        f"{what}: {got.numel()} bytes, oracle has {want.numel()}"
    diff = (got != want).nonzero().flatten()
    assert diff.numel() == 0, (
        f"{what}: {diff.numel()} bytes differ from the CPU oracle, "
        f"first offsets {diff[:8].tolist()}")


def assert_bits(got, want, what):
    """Bit-for-bit equality of two 16-bit float tensors (-0.0 != 0.0)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    diff = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert diff.numel() == 0, (
        f"{what}: {diff.shape[0]} values differ from the CPU oracle, "
        f"first at {diff[:4].tolist()}")


# ---- the fp16 double-rounding trap ------------------------------------------

_tie = {}


def fp16_tie_amaxes():
    """Positive finite fp16 amax values (as fp16 bit patterns, int64) for
    which magnitude m in (1.5, 3.0) times scale = amax/6 rounds differently
    in one step (f64 product -> fp16) than in two (f32 product -> fp16).
    Returns {1.5: bits, 3.0: bits}; numpy does the roundings, because its
    float64 -> float16 cast is a single correct rounding."""
    if "amax" not in _tie:
        bits = np.arange(1, 0x7c00, dtype=np.uint16)
        amax = bits.view(np.float16).astype(np.float32)
        scale = amax / np.float32(6.0)
        out = {}
        for m in (1.5, 3.0):
            two = (np.float32(m) * scale).astype(np.float16)
            one = (np.float64(m) * scale.astype(np.float64)).astype(np.float16)
            out[m] = torch.from_numpy(
                bits[two.view(np.uint16) != one.view(np.uint16)]
                .astype(np.int64))
        _tie["amax"] = out
    return _tie["amax"]


def make_tie_page():
    """One fp16 tile (1, TIE_TILE_BYTES/2) of G=16 groups: one group per tie
    amax, holding the amax and, where they exist, one input x <= amax that
    encodes to magnitude 1.5 and one that encodes to 3.0; zero padding."""
    if "page" not in _tie:
        ties = torch.cat(list(fp16_tie_amaxes().values())).sort().values
        n = TIE_TILE_BYTES // 2
        assert ties.numel() * 16 <= n
        page = torch.zeros(n // 16, 16, dtype=torch.float16)
        top = int(ties.max())
        cand = torch.arange(1, top + 1, dtype=torch.int16).view(torch.float16)
        amax = ties.to(torch.int16).view(torch.float16).float()[:, None]
        inv = torch.div(torch.full_like(amax, E2M1_MAX), amax)
        mag = encode(cand.float()[None, :] * inv)
        mag[cand.float()[None, :] > amax] = 0xff
        page[:ties.numel(), 0] = amax[:, 0].half()
        for slot, code in ((1, 3), (2, 5)):
            hit = mag == code
            has = hit.any(1)
            first = hit.int().argmax(1)
            page[:ties.numel(), slot] = torch.where(
                has, cand[first], torch.zeros((), dtype=torch.float16))
        _tie["page"] = page.reshape(1, n)
    return _tie["page"]


def single_rounding_y(x, group_size):
    """What a fused product-and-cast would load instead of the oracle's y:
    value(code) * scale as an exact f64 product, rounded ONCE to fp16."""
    codes, scale, _, _ = oracle(x, group_size)
    lead, n = x.shape[:-1], x.shape[-1]
    c = codes.reshape(*lead, n // group_size, group_size)
    lut = torch.tensor(MAGNITUDES, dtype=torch.float64)
    val = lut[(c & 7).long()]
    val = torch.where((c & 8) != 0, -val, val)
    prod = (val * scale.double()[..., None]).numpy()
    return torch.from_numpy(prod.astype(np.float16)).reshape(*lead, n)


# ---- hand-built slab holding every code byte --------------------------------

def all_codes_slab(scales):
    """Records of 1024-byte tiles at G=16 (512 elements = 32 groups = 256
    code bytes): tile i holds every code byte 0..255 once, all of its
    groups scaled by scales[i] (f32). Returns (slab uint8 1-D, codes uint8
    (tiles, 512), scale f32 (tiles, 32))."""
    scales = scales.to(torch.float32)
    tiles = scales.numel()
    packed = torch.arange(256, dtype=torch.uint8).expand(tiles, 256)
    scale = scales[:, None].expand(tiles, 32).contiguous()
    slab = torch.cat([packed, scale.view(torch.uint8).reshape(tiles, 128)],
                     dim=1).reshape(-1).contiguous()
    return slab, unpack_codes(packed), scale


def decode_scales(dtype):
    """A spread of f32 scales amax/6 for the exhaustive decode: amax =
    2^k (1 + j/8) across the page type's range, and every fp16 tie amax."""
    if dtype == torch.float16:
        ks = range(-22, 16, 3)
    else:
        ks = range(-120, 121, 16)
    amax = [2.0 ** k * (1 + j / 8) for k in ks for j in (0, 3, 5, 7)]
    ties = torch.cat(list(fp16_tie_amaxes().values()))
    amax = torch.cat([torch.tensor(amax, dtype=torch.float32),
                      ties.to(torch.int16).view(torch.float16).float()])
    return torch.div(amax, torch.full_like(amax, E2M1_MAX))


# ---- every finite bit pattern as x -------------------------------------------

_LADDER = {
    torch.bfloat16: (2.0 ** -100 * 1.25, 2.0 ** -40 * 1.171875, 0.8125,
                     1792.0, 2.0 ** 60 * 1.5),
    torch.float16: (2.0 ** -20 * 1.25, 2.0 ** -8 * 1.171875, 0.8125, 48.5,
                    1792.0),
}
# bf16 amax below this is out of scope (6/amax overflows f32 under ~1.8e-38)
_MIN_AMAX = {torch.bfloat16: 2.0 ** -120, torch.float16: 2.0 ** -24}
_exhaustive = {}


def exhaustive_groups(dtype):
    """Every finite bit pattern of dtype as x, in G=16 groups [amax, 15 x].
    Patterns are sorted by magnitude and taken 15 at a time; each run is
    stored once per amax: its own largest magnitude m, about 1.3 m, 2.7 m
    and 6.5 m, and every entry >= m of a fixed ladder that holds values
    below and above 1. Returns (x (groups, 16), m per run, the amax values
    each run met (runs, 9), NaN where a ladder entry was too small)."""
    if dtype not in _exhaustive:
        bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
        x = bits.view(dtype)
        x = x[torch.isfinite(x.float())]
        assert x.numel() == 65536 - (256 if dtype == torch.bfloat16 else 2048)
        x = x[x.float().abs().argsort(stable=True)]
        pad = (-x.numel()) % 15
        x = torch.cat([x, x[-1:].expand(pad)]).reshape(-1, 15)
        top = x.float().abs().amax(1)
        fmax = torch.finfo(dtype).max
        groups, seen = [], []
        for r in (1.0, 1.3125, 2.6875, 6.5):
            a = (top * r).clamp(_MIN_AMAX[dtype], fmax).to(dtype)
            a = torch.maximum(a.float(), top).to(dtype)  # rounding kept it
            groups.append(torch.cat([a[:, None], x], dim=1))
            seen.append(a.float())
        for a in _LADDER[dtype]:
            keep = top <= a
            col = torch.full((int(keep.sum()), 1), a).to(dtype)
            assert col.float()[0, 0].item() == a  # representable
            groups.append(torch.cat([col, x[keep]], dim=1))
            seen.append(torch.where(keep, torch.tensor(a), torch.nan))
        _exhaustive[dtype] = (torch.cat(groups), top, torch.stack(seen, 1))
    return _exhaustive[dtype]


def wait_finished(handler, n=1, timeout=30.0):
    out = []
    deadline = time.time() + timeout
    while len(out) < n and time.time() < deadline:
        out.extend(handler.get_finished())
        time.sleep(0.002)
    assert len(out) >= n, f"only {len(out)} of {n} jobs finished"
    return out
