"""CPU oracle and heterogeneous input for serialize="fp8_e4m3_group".

Shared by test_fp8_group.py (host mode) and test_fp8_group_gpu.py (HIP
kernels): both must produce exactly these bytes — that equality is the
contract between files written on a GPU and files written in host mode.

Arithmetic per G-element group, all in f32 (docs/architecture.md):
  amax = max|x|, 0 -> 1;  scale = amax / 448 (stored);  inv = 448 / amax;
  q = RNE_e4m3fn(x * inv);  y = bf16_RNE(f32(q) * scale).

`inv` is a true f32 division, spelled torch.div on two tensors. The Python
expression ``448.0 / amax`` on a tensor is NOT that: Tensor.__rtruediv__
evaluates ``amax.reciprocal() * 448.0``, two roundings, which differs from
the division in the last bit for about a quarter of all amax values and
would make the oracle disagree with the normative step above.
"""
import time

import torch

E4M3_MAX = 448.0
# |y - x| <= REL_BOUND * group_amax, derived: the scaled value x*inv lies in
# [-448, 448], where the widest e4m3 ulp is 32 (binade [256, 448]), so the
# quantization error is at most 16 = 2^-4 * 256 <= 448/28, i.e. 0.0357 of
# group_amax; bf16 rounding of y adds at most 2^-9 * |y| and the f32
# roundings ~2^-23. 0.07 is the bound the per-tile tests use per tile; here
# it applies per group.
REL_BOUND = 0.07


def make_pages(num_blocks, block_bytes, group_size, num_layers, seed):
    """Per-layer bf16 pages (num_blocks, block_bytes/2): randn with each
    group scaled by 10**U(-3, 2), plus in every tile one all-zero group
    and one group holding exactly representable values (+-448*s, 0.5*s,
    with s = 2^-3 the resulting group scale)."""
    n = block_bytes // 2
    ng = n // group_size
    assert n % group_size == 0 and ng >= 3
    gen = torch.Generator().manual_seed(seed)
    s = 0.125
    pages = []
    for _ in range(num_layers):
        x = torch.randn(num_blocks, ng, group_size, generator=gen)
        x *= 10.0 ** (torch.rand(num_blocks, ng, 1, generator=gen) * 5 - 3)
        blocks = torch.arange(num_blocks)
        x[blocks, blocks % ng] = 0.0               # an all-zero group
        exact = (blocks + 1) % ng                  # a different group
        x[blocks, exact] = torch.randn(num_blocks, group_size,
                                       generator=gen) * s
        x[blocks, exact, 0] = E4M3_MAX * s
        x[blocks, exact, 1] = -E4M3_MAX * s
        x[blocks, exact, 2] = 0.5 * s
        pages.append(x.reshape(num_blocks, n).to(torch.bfloat16))
    return pages


def oracle(x, group_size):
    """x: bf16 (..., n). Returns (q uint8 (..., n), scales f32 (..., n/G),
    y bf16 (..., n), amax f32 (..., n/G))."""
    lead, n = x.shape[:-1], x.shape[-1]
    xg = x.float().reshape(*lead, n // group_size, group_size)
    amax = xg.abs().amax(-1, keepdim=True)
    amax = torch.where(amax == 0, torch.ones_like(amax), amax)
    inv = torch.div(torch.full_like(amax, E4M3_MAX), amax)
    scale = torch.div(amax, torch.full_like(amax, E4M3_MAX))
    q = (xg * inv).to(torch.float8_e4m3fn)
    y = (q.float() * scale).to(torch.bfloat16)
    return (q.view(torch.uint8).reshape(*lead, n),
            scale.reshape(*lead, n // group_size),
            y.reshape(*lead, n),
            amax.reshape(*lead, n // group_size))


def oracle_records(pages, ids, group_size):
    """Expected file/slab bytes for blocks `ids`: records
    [n fp8 | n/G f32 scales], block-major, layer-minor. uint8 1-D."""
    recs = []
    for page in pages:
        q, scale, _, _ = oracle(page[ids].cpu(), group_size)
        recs.append(torch.cat(
            [q, scale.contiguous().view(torch.uint8).reshape(len(ids), -1)],
            dim=1))
    return torch.stack(recs, dim=1).reshape(-1)


def record_bytes(block_bytes, group_size):
    n = block_bytes // 2
    return n + 4 * n // group_size


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


def wait_finished(handler, n=1, timeout=30.0):
    out = []
    deadline = time.time() + timeout
    while len(out) < n and time.time() < deadline:
        out.extend(handler.get_finished())
        time.sleep(0.002)
    assert len(out) >= n, f"only {len(out)} of {n} jobs finished"
    return out
