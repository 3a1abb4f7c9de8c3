"""Philox4x32-10 in plain numpy, for the oracles that share no code with the
backends (test_qkey_tournament.py, test_perm_oracle.py)."""
import numpy as np

U64 = np.uint64
MASK = U64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counter words; 32-bit values held in uint64."""
    c = [np.asarray(x, dtype=U64) & MASK for x in (c0, c1, c2, c3)]
    k0, k1 = U64(k0) & MASK, U64(k1) & MASK
    for _ in range(10):
        p0 = U64(0xD2511F53) * c[0]
        p1 = U64(0xCD9E8D57) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> U64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + U64(0x9E3779B9)) & MASK
        k1 = (k1 + U64(0xBB67AE85)) & MASK
    return c
