"""Shared helpers for the parity tests (test infrastructure)."""
import numpy as np


def rand_poly(rng, moduli, nlimb_mods, N):
    return np.stack([rng.integers(0, moduli[m], N, dtype=np.uint64) for m in nlimb_mods])


def rand_ct(rng, moduli, level, N, B=1):
    out = np.zeros((B, 2, level + 1, N), dtype=np.uint64)
    for b in range(B):
        for c in range(2):
            for j in range(level + 1):
                out[b, c, j] = rng.integers(0, moduli[j], N, dtype=np.uint64)
    return out


def plant_runs(x, moduli):
    """Constant runs at the head of every limb of x [..][limbs][N] (limb j mod
    moduli[j]): 16 coefficients of 0, 16 of 1, 16 of q - 1, so that additions,
    subtractions and products wrap at both ends.  In place; returns x."""
    for j in range(x.shape[-2]):
        x[..., j, 0:16] = 0
        x[..., j, 16:32] = 1
        x[..., j, 32:48] = moduli[j] - 1
    return x


def round_half_away(x):
    """round-half-away-from-zero of an exact rational, as a Python int (the
    rule of the evaluator's scalar constants)."""
    from fractions import Fraction
    x = Fraction(x)
    return -int(-x + Fraction(1, 2)) if x < 0 else int(x + Fraction(1, 2))


def _rand_below(rng, n):
    """a Python int in [0, n), n of any size (64 spare bits: no visible bias)"""
    return int.from_bytes(rng.bytes((n.bit_length() + 7) // 8 + 8), "little") % n


def _rand_bitlen(rng, maxbits):
    """a Python int whose bit length is uniform in 0..maxbits (0 gives 0, 1 gives 1)"""
    b = int(rng.integers(0, maxbits + 1))
    return 0 if b == 0 else (1 << (b - 1)) | _rand_below(rng, 1 << (b - 1))


def digit_limbs(level, K):
    """the Q limbs of every gadget digit at `level`: digit i holds [iK, min((i+1)K, level+1))"""
    return [list(range(lo, min(lo + K, level + 1))) for lo in range(0, level + 1, K)]


def plant_digit_values(rng, moduli, level, K, N):
    """Coefficient-domain limbs w [level+1][N] (limb j mod moduli[j]; moduli =
    the Q primes then the K special primes) whose gadget digits are integers on
    the rounding edges of the basis extension, and those integers X[digit][n]
    (Python ints, 0 <= X < S_i = the product of digit i's primes; limb j of the
    digit holds X mod q_j).  Per digit, coefficient n takes class (n + 3i) mod 8:
      0-2  X = delta, delta's bit length uniform in 0..min(50, bitlen(S_i) - 2):
           the float64 quotient sum sits just above an integer;
      3-5  X = S_i - 1 - delta: just below one;
      6    X = k t + r, t a QP modulus outside the digit (round-robin), r one of
           0, 1, t - 1, t // 2, t // 2 +- 1: target t's reduction on its edges
           (as 0-2 when S_i <= t);
      7    uniformly random (the control).
    A digit of one limb takes the centred path (v = x >= s >> 1) instead: 0, 1,
    s // 2 - 1, s // 2, s // 2 + 1, s - 1 in turn, and the same control."""
    nq = len(moduli) - K
    w = np.zeros((level + 1, N), dtype=np.uint64)
    X = []
    for i, limbs in enumerate(digit_limbs(level, K)):
        S = 1
        for j in limbs:
            S *= moduli[j]
        targets = [moduli[j] for j in range(level + 1) if j not in limbs] + list(moduli[nq:])
        dbits = min(50, S.bit_length() - 2)
        xs, nc = [], 0
        for n in range(N):
            cls = (n + 3 * i) % 8
            t = 0
            if cls == 6 and len(limbs) > 1:
                t = targets[nc % len(targets)]
                r = (0, 1, t - 1, t // 2, t // 2 - 1, t // 2 + 1)[nc // len(targets) % 6]
                nc += 1
            if cls == 7:
                x = _rand_below(rng, S)
            elif len(limbs) == 1:
                x = (0, 1, S // 2 - 1, S // 2, S // 2 + 1, S - 1)[(n // 8 * 7 + cls) % 6]
            elif S > t > 0:
                kmax = (S - 1 - r) // t
                x = min(_rand_bitlen(rng, kmax.bit_length()), kmax) * t + r
            elif cls < 3 or cls == 6:
                x = _rand_bitlen(rng, dbits)
            else:
                x = S - 1 - _rand_bitlen(rng, dbits)
            assert 0 <= x < S
            xs.append(x)
        X.append(xs)
        for j in limbs:
            w[j] = np.array([x % moduli[j] for x in xs], dtype=np.uint64)
    return w, X


def decode_edge_values(rng, qs):
    """Centred representatives of residues mod Q = prod qs (x <= (Q - 1) / 2 is
    itself, above that x - Q) on the edges of the decoder's CRT, conversion
    and centring, as Python ints: (named specials, sweep).  Specials:
    0, +-1; ties of the one-word conversion; the word boundary; ties of the
    two-word conversion with and without a sticky bit, top word normalised
    (lz == 0) or not; each side of the centring comparison; Q - 1; values
    where a Garner digit or the Q - x loop carries; values whose top digits
    are 0.  Sweep: both signs of a random value of every bit length up to
    bitlen(Q) - 2.  Values that do not fit |x| <= (Q - 1) / 2 are left out (a
    short chain has no two-word values)."""
    Q = 1
    for q in qs:
        Q *= q
    half = (Q - 1) // 2

    def centred(r):
        r %= Q
        return r if r <= half else r - Q

    sp = [0, 1, -1, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1]
    for top in (2 ** 63 + 2 ** 10, 2 ** 62 + 2 ** 9):
        sp += [top << 64, (top << 64) + 1]
    sp += [-x for x in sp[3:]]
    sp = [x for x in sp if abs(x) <= half]
    sp += [half, centred(half + 1), centred(Q - 1), centred(qs[0]), centred(Q - qs[0])]
    if len(qs) > 1:
        sp += [centred(qs[0] * qs[1] - 1), centred(Q - qs[0] * qs[1]), centred(qs[0] * qs[1])]
    if len(qs) > 2:  # top digits 0, of either sign
        sp += [qs[0] * qs[1] // 3, -(qs[0] * qs[1] // 3), qs[0] - 1, -(qs[0] - 1)]
    sweep = []
    for b in range(1, Q.bit_length() - 1):
        x = (1 << (b - 1)) | _rand_below(rng, 1 << (b - 1))
        sweep += [x, -x]
    assert all(-half <= x <= half for x in sp + sweep)
    return sp, sweep


def constant_rows(xs, qs, N):
    """[len(xs)][len(qs)][N]: image b is the NTT of the constant polynomial
    xs[b], the constant row xs[b] mod q_j"""
    out = np.zeros((len(xs), len(qs), N), dtype=np.uint64)
    for b, x in enumerate(xs):
        for j, q in enumerate(qs):
            out[b, j, :] = x % q
    return out


SMALL = dict(logn=13, logq=[55, 40, 40, 40, 40, 40], logp=[60, 60])

# the chains (and levels) of the planted basis-extension parity tests
# (test_gpu_bext_planted.py; their CPU guards in test_oracle.py)
PLANT_CHAINS = {
    "small": dict(logn=13, logq=SMALL["logq"], logp=SMALL["logp"], levels=[5, 1]),  # K = 2: <2>, lazy targets
    "k4": dict(logn=13, logq=[60] + [40] * 7, logp=[60] * 4, levels=[7]),  # <4>
    # digits of 8, 3 and 1 limbs; 30-bit sources and targets beside 60/61-bit ones: NARROW, WT, NT, LAZY
    "k8": dict(logn=13, logq=[60] + [30] * 16, logp=[61] * 8, levels=[16, 10, 8]),
    "k1": dict(logn=13, logq=[60] + [40] * 5, logp=[61], levels=[5]),  # every digit centred
    "n15": dict(logn=15, logq=[60, 40, 40, 40, 40, 40], logp=[60, 60], levels=[5]),  # the NTT-prologue paths
}


class SchemeCache:
    """A GPU scheme shared by the tests of a module, rebuilt whenever another
    test has replaced or deleted the process-global scheme since (the library
    keeps one scheme per process, like Lattigo's scheme.go:32), so the tests
    pass in any order or -k selection."""

    def __init__(self):
        self.val = None

    def get(self, make):
        if self.val is None or not self.val[0].scheme_current():
            self.val = None
            self.val = make()
        return self.val


def bootstrap_keys(lib, ns):
    """The keys of the bootstrapper for `ns` slots (relinearisation, Galois,
    EvkDenseToSparse, EvkSparseToDense): with the input ciphertext, the only
    inputs the CPU oracle shares with the library.  Everything else in the
    circuit -- the prime chain, F, K, the cosine coefficients, the
    CoeffsToSlots / SlotsToCoeffs diagonals and their encoding, the trace
    elements -- the oracle derives itself (oracle.BtpCircuit)."""
    return dict(rlk=lib.bootstrap_export(ns, "rlk"), d2s=lib.bootstrap_export(ns, "d2s"),
                s2d=lib.bootstrap_export(ns, "s2d"),
                gks={int(g): lib.bootstrap_export(ns, "galois", int(g)) for g in lib.bootstrap_export(ns, "galois_keys")})


def bootstrap_oracle(oracle_mod, lib, logn, log_scale, ns, logp):
    """(bootstrapping-chain Oracle, BtpCircuit) derived by the oracle from the
    scheme's moduli and logPs; checks the library's chain is the same."""
    sm = lib.moduli()
    bq, bp = oracle_mod.btp_chain(logn, sm, lib.L, logp)
    lq, lp = lib.bootstrap_moduli(ns)
    assert (lq, lp) == (bq, bp), "the library's bootstrapping chain differs from the oracle's"
    boot = oracle_mod.Oracle(logn, bq + bp, len(bq), len(bp))
    return boot, oracle_mod.BtpCircuit(boot, log_scale, ns)
