"""Pure numpy oracle of the per-record checksum format (docs/architecture.md).

A checksummed record is [ payload (P bytes, P % 4 == 0) | footer ]:

  footer bytes 0..7    sum            u64, little-endian
         bytes 8..11   magic          0x5343564B (the bytes K V C S)
         bytes 12..15  payload_bytes  P as u32

  x_i = ((i + 1) << 32) | w[i]        w = payload as little-endian u32 words
  h(x): x ^= x >> 30; x *= 0xbf58476d1ce4e5b9;
        x ^= x >> 27; x *= 0x94d049bb133111eb;
        x ^= x >> 31                  (mod 2^64)
  sum = SUM_i h(x_i) mod 2^64

Shared by test_checksum.py (host mode) and test_checksum_gpu.py (HIP
kernels): host mode, the staged path and the zero-copy path must all write
exactly the bytes built here from the payload bytes.
"""
import time

import numpy as np

MAGIC = 0x5343564B
FOOTER = 16

# (payload, sum) computed with plain Python integers and cross-checked with
# the vectorised version below
GOLDEN = [
    (bytes(16), 0x3524886FA1F89CD1),
    (bytes(k & 0xFF for k in range(388)), 0x784AA003648E06C0),
    (bytes((k * 7 + 3) & 0xFF for k in range(768)), 0xAC68543EDCFF8E63),
]


def _words(payload):
    a = np.frombuffer(bytes(payload), dtype=np.uint8)
    assert a.size % 4 == 0, "payload length must be a multiple of 4"
    return a.view("<u4").astype(np.uint64)


def checksum(payload):
    """sum over the payload (bytes-like), as a Python int."""
    w = _words(payload)
    with np.errstate(over="ignore"):
        x = ((np.arange(1, w.size + 1, dtype=np.uint64)) << np.uint64(32)) | w
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
        return int(x.sum(dtype=np.uint64))


def checksum_python(payload):
    """The same sum with plain Python integers (slow; golden values only)."""
    b = bytes(payload)
    m = (1 << 64) - 1
    total = 0
    for i in range(len(b) // 4):
        x = ((i + 1) << 32) | int.from_bytes(b[4 * i:4 * i + 4], "little")
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & m
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & m
        x ^= x >> 31
        total = (total + x) & m
    return total


def footer(payload):
    """The 16 footer bytes of a record with this payload."""
    return (checksum(payload).to_bytes(8, "little")
            + MAGIC.to_bytes(4, "little")
            + len(bytes(payload)).to_bytes(4, "little"))


def seal(plain, payload_bytes):
    """Expected checksummed slab/file for the bytes a checksum=False engine
    wrote (`plain`: whole records of payload_bytes each)."""
    plain = bytes(plain)
    assert len(plain) % payload_bytes == 0
    out = bytearray()
    for off in range(0, len(plain), payload_bytes):
        rec = plain[off:off + payload_bytes]
        out += rec
        out += footer(rec)
    return bytes(out)


def payloads(sealed, payload_bytes):
    """Strip the footers again: the concatenated payload slices."""
    sealed = bytes(sealed)
    stride = payload_bytes + FOOTER
    assert len(sealed) % stride == 0
    return b"".join(sealed[off:off + payload_bytes]
                    for off in range(0, len(sealed), stride))


def verify(sealed, payload_bytes):
    """(bad records, first bad index or -1) of a checksummed slab."""
    sealed = bytes(sealed)
    stride = payload_bytes + FOOTER
    bad, first = 0, -1
    for t, off in enumerate(range(0, len(sealed), stride)):
        rec = sealed[off:off + payload_bytes]
        if sealed[off + payload_bytes:off + stride] != footer(rec):
            bad += 1
            if first < 0:
                first = t
    return bad, first


def payload_bytes(serialize, block_bytes, group_size=128):
    n = block_bytes // 2
    if serialize == "raw":
        return block_bytes
    if serialize == "fp8_e4m3":
        return n + 4
    assert serialize == "fp8_e4m3_group"
    return n + 4 * n // group_size


def wait_finished(handler, n=1, timeout=30.0):
    out = []
    deadline = time.time() + timeout
    while len(out) < n and time.time() < deadline:
        out.extend(handler.get_finished())
        time.sleep(0.002)
    assert len(out) >= n, f"only {len(out)} of {n} jobs finished"
    return out
