"""Test-local reference of the device noise source: Philox4x32-10 in numpy with uint64 products, the exact fp32
uniforms and a float64 Box-Muller from the same words.  Imports nothing from the product; pinned by the Random123 known answers
(tests/test_noise_cpu.py)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter = 4 and key = 2 arrays (or ints) of 32-bit words, broadcast together -> the 4 output words as uint64 arrays < 2^32."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & MASK for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # < 2^64: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return c


def uniform(w):
    """u = ((w >> 9) + 0.5) * 2^-23 in float64: 24 significant bits, so also the exact fp32 value."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def item_words(seed, stream, n_groups):
    """The words of one item's groups q = 0 .. n_groups - 1 as uint64 [n_groups][4]: key = seed, counter = (q, 0, stream_lo, stream_hi)."""
    seed, stream = int(seed), int(stream)
    q = np.arange(n_groups, dtype=np.uint64)
    return np.stack(philox4x32_10((q, 0, stream & 0xFFFFFFFF, stream >> 32), (seed & 0xFFFFFFFF, seed >> 32)), axis=1)


def item_uniform(seed, stream, n_rows, n_mel):
    """float64 [n_rows][n_mel]: element e = t * n_mel + m takes word e & 3 of group e >> 2."""
    assert n_mel % 4 == 0
    return uniform(item_words(seed, stream, n_rows * n_mel // 4)).reshape(n_rows, n_mel)


def item_normal(seed, stream, n_rows, n_mel):
    """-> (z, r) float64 [n_rows][n_mel]: Box-Muller on the word pairs (0, 1) and (2, 3), z = r cos / sin (2 pi u_odd), r = sqrt(-2 ln u_even)
    broadcast to both elements of its pair."""
    u = item_uniform(seed, stream, n_rows, n_mel).reshape(-1, 2)
    r = np.sqrt(-2.0 * np.log(u[:, 0]))
    ang = 2.0 * np.pi * u[:, 1]
    z = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    return z.reshape(n_rows, n_mel), np.repeat(r, 2).reshape(n_rows, n_mel)


def fill(keys, seq_len, N, n_mel, kind):
    """What vv_noise_fill writes, in float64: [B][N][n_mel], rows past clamp(seq_len[b], 0, N) zero; kind 0 -> (z, r), kind 1 -> u."""
    B = len(keys)
    out, rr = np.zeros((B, N, n_mel)), np.zeros((B, N, n_mel))
    for b in range(B):
        n = max(0, min(int(seq_len[b]), N))
        if kind == 1:
            out[b, :n] = item_uniform(keys[b][0], keys[b][1], n, n_mel)
        else:
            out[b, :n], rr[b, :n] = item_normal(keys[b][0], keys[b][1], n, n_mel)
    return out if kind == 1 else (out, rr)
