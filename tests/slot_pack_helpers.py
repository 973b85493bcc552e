"""Reference pieces of the slot-packing tests (test infrastructure): monomials and their NTTs, the pack and
unpack compositions over Oracle.mul_coeffs, and oracle-made keys for the oracle's bootstrapping circuit."""
import numpy as np


def brv(j, bits):
    return int(format(j, "0%db" % bits)[::-1], 2)


def unit(N, k, q):
    """X^k mod (X^N + 1, q), k mod 2N"""
    k %= 2 * N
    u = np.zeros(N, dtype=np.uint64)
    u[k % N] = 1 if k < N else q - 1
    return u


def mono(orc, k, nl):
    """M_k [nl][N]: the oracle's forward NTT of X^k, limb by limb"""
    return np.stack([orc.ntt(j, unit(orc.N, k, orc.moduli[j])) for j in range(nl)])


def pack(orc, x, g):
    """x [B][..][nl][N] -> [ceil(B / g)][..][nl][N]: out_k = sum_i M_i o x_(k + i h)"""
    B, nl = x.shape[0], x.shape[-2]
    h = -(-B // g)
    q = np.array(orc.moduli[:nl], dtype=np.uint64)[:, None]
    out = x[:h].copy()
    for i in range(1, g):
        m = mono(orc, i, nl)
        for k in range(h):
            if k + i * h < B:
                t = np.stack([orc.mul_coeffs(r, m, list(range(nl))) for r in x[k + i * h].reshape(-1, nl, orc.N)])
                out[k] = (out[k] + t.reshape(out[k].shape)) % q  # residues below 2^61: the sum fits
    return out


def unpack(orc, y, g, B):
    """y [h][..][nl][N] -> [B][..][nl][N]: out_(k + i h) = M_-i o y_k"""
    h, nl = y.shape[0], y.shape[-2]
    assert h == -(-B // g)
    out = np.zeros((B,) + y.shape[1:], dtype=np.uint64)
    for i in range(g):
        m = mono(orc, -i, nl)
        for k in range(h):
            if k + i * h < B:
                t = np.stack([orc.mul_coeffs(r, m, list(range(nl))) for r in y[k].reshape(-1, nl, orc.N)])
                out[k + i * h] = t.reshape(y[k].shape)
    return out


# (tests/test_oracle.py keeps the same recipe as _btp_keys for its own test: the two must stay in step)
def btp_test_keys(o, sk, circ, seed):
    """Keys the oracle makes for its own circuit (the recipe of test_oracle_bootstrap_functional):
    relinearisation, every Galois key the circuit uses (BSGS babies / giants, trace, conjugation), and the
    ephemeral secret's two switching keys."""
    N, n = o.N, o.N // 2
    gels = {2 * N - 1}
    p = circ.params()
    gels |= {o.galois_element(int(p["slots"]) << i) for i in range(int(p["ntrace"]))}
    for k in range(int(p["nlt"])):
        _, n1, idx, _ = circ.lt(k)
        for d in idx:
            giant, baby = ((d // n1) * n1) % n, d % n1
            gels |= {o.galois_element(r) for r in (giant, baby) if r}
    keys = dict(rlk=o.gen_evk(seed, o.mul_coeffs(sk, sk, list(range(o.L + o.K))), sk), gks={})
    for i, g in enumerate(sorted(gels)):
        keys["gks"][g] = o.gen_evk(seed + 1 + i, sk, o.automorphism_ntt(sk, pow(g, -1, 2 * N)))
    se = o.gen_secret(seed + 999, 32)
    keys["d2s"] = o.gen_evk(seed + 1000, sk, se)
    keys["s2d"] = o.gen_evk(seed + 1001, se, sk)
    return keys
