"""The key-switch and diagonal multiply-accumulate kernels at the bounds of
their unreduced accumulators (csrc/common.h MacAcc, mac_reduce_small,
macw_reduce8, MacD; csrc/kernels.hip ks_mac_body, ks_mac_hoisted_kernel,
gadget_at, lt_bsgs_body, lt_giant_kernel).

With uniformly random operands every partial sum sits near half of its
maximum, so a carry dropped at 2^64, a float64 sum rounded at 2^53, a Barrett
estimate that is low by 3, or a flush one giant late passes a random test.
Here every operand is planted through the unchanged C-ABI:
  * the ciphertext: helpers.max_digit_ct, one image per attacked limb t, whose
    gadget digits are all t - 1 on that limb at every position (K = 1: every
    digit on every limb at once), asserted first on the oracle alone
    (helpers.digits_at_max);
  * the keys: the "max key", q_m - 1 in every digit, component and modulus on
    a seeded half M of the positions (read through the automorphism: see
    helpers.key_mask) and the generated key elsewhere, loaded with
    LoadRotationKey; the relinearisation key likewise through the key bundle;
  * the diagonals: q_m - 1 on M, random residues elsewhere, loaded with
    LoadPlaintextDiagonal into a transform made in "load" mode.
On M every counted product is (q - 1)^2 and every addend q - 1.  All
comparisons are bit for bit against the CPU oracle with the exported
(planted) keys and diagonals; tests/test_planted_mac.py checks the oracle
itself at these values against Python integers.

What each case fills (EDGE: 60, 48, 49, 52, 54, 40, 41, 41-bit Q limbs and
two 61-bit P limbs, a limb on each side of every path switch):
  a  ks_mac_body: KS_CH = 2 products per MacAcc, beta = 4, 3, 16
  b  ks_mac_hoisted_kernel<4> with beta = 4 and <8> with beta = 8 full, the
     grouped fallback at beta = 9
  c  lt_giant_kernel: 4 of 4 products per MacAcc on the 54/60/61-bit limbs
     (one image per launch), 120 of 120 terms in the small accumulator on the
     40..52-bit limbs (24 giants of 4 products and the P c0 addend at level 7,
     30 giants of 3 and the addend at level 5)
  d  the relinearisation's ks_mac_body
  e  lt_bsgs_body: 7 of 8 and 15 of 16 slots of MacD (40/41/48 bits), 7 and
     8 + 7 of macw_reduce8's 8 (49..60 bits), 4 + 3 and 4 + 4 + 4 + 3 of
     MacAcc's 4 (61 bits)
  f  gadget_at inside lt_bsgs_body: 4 of 4 products per MacAcc"""
import numpy as np
import pytest

from tests.helpers import (EDGE_BITS, LT_IDX, MAC_CHAINS, SchemeCache, bsgs_split, digit_limbs, digits_at_max,
                           expected_digits, key_mask, load_galois_key_words, load_max_galois_key, max_digit_ct,
                           max_key, max_mask, mform, neg_pinv_rows, plant_relin_key, qp_blob, rand_poly,
                           share_at_max, sum_expected)

pytestmark = pytest.mark.gpu

SCALE = 2.0 ** 40
SEED = 6161
MAXHOIST = 16  # keys per ks_mac_hoisted launch (test_gpu_hoisted.py reads it from hoist.h)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


class Env:
    def __init__(self, oracle_mod, name):
        from orion_amd.backend import HipLibrary
        ch = MAC_CHAINS[name]
        self.lib = HipLibrary().new_scheme(ch["logn"], ch["logq"], ch["logp"], 40, h=192, seed=SEED)
        self.lib.GenerateSecretKey()
        self.lib.GeneratePublicKey()
        self.lib.GenerateRelinearizationKey()
        self.mods = self.lib.moduli()
        self.orc = oracle_mod.Oracle(ch["logn"], self.mods, len(ch["logq"]), len(ch["logp"]))
        self.M = max_mask(self.orc.N)
        assert self.M.mean() >= 0.25
        self.keys = {}  # g -> (kind, the key as loaded and exported)
        self.refs = {}  # references shared by the cases of a parametrised test

    def g(self, amount):
        return int(self.lib.GaloisElement(int(amount)))

    def cached(self, tag, keys, make):
        """make()'s value, kept for as long as the keys it was made under are the loaded ones"""
        old = self.refs.get(tag)
        if old is None or set(old[0]) != set(keys) or any(old[0][g] is not keys[g] for g in keys):
            self.refs[tag] = (dict(keys), make())
        return self.refs[tag][1]

    def _keys(self, gels, kind, load):
        for g in gels:
            if g != 1 and self.keys.get(g, ("", None))[0] != kind:
                self.keys[g] = (kind, load(g))
        return {g: self.keys[g][1] for g in gels if g != 1}

    def max_keys(self, gels):
        """the max keys of gels; every one of them meets M after its automorphism"""
        out = self._keys(gels, "max", lambda g: load_max_galois_key(self.lib, self.orc, g, self.M))
        assert share_at_max(self.orc, {g: key_mask(self.orc, self.M, g) for g in out}) == self.M.mean()
        for g, k in out.items():
            mk = key_mask(self.orc, self.M, g)
            for m in self.orc.qp_mods(self.orc.L - 1):
                assert np.all(k[:, :, m][:, :, mk] == self.mods[m] - 1)
        return out

    def own_keys(self, gels):
        """freshly generated keys, as the scheme makes them"""
        def load(g):
            blob, _ = self.lib.GenerateAndSerializeRotationKey(g)
            self.lib.LoadRotationKey(blob, g)
            return self.lib.export_galois_key(g)
        return self._keys(gels, "own", load)

    def digit0_keys(self, gels):
        """word 1 in digit 0, both components, 0 elsewhere: the gadget product is
        (D_0, D_0), the digit-0 extension of c1"""
        nl = self.orc.L + self.orc.K
        words = [[[int(d == 0)] * nl for _ in range(2)] for d in range(self.orc.dnum)]
        return self._keys(gels, "digit0", lambda g: load_galois_key_words(self.lib, self.orc, g, words))

    def images(self, level, c0):
        """(targets, x [T][2][level+1][N]): one max_digit_ct image per attacked
        limb (K = 1: one image for all), the digit count asserted on the oracle.
        c0: "negpinv", "zero" or a Generator for random rows."""
        orc = self.orc
        targets = orc.qp_mods(level) if orc.K > 1 else [0]
        x = []
        for t in targets:
            if c0 == "negpinv":
                r = neg_pinv_rows(orc, level)
            elif c0 == "zero":
                r = None
            else:
                r = rand_poly(c0, self.mods, list(range(level + 1)), orc.N)
            x.append(max_digit_ct(orc, level, t, r))
            for tt in (orc.qp_mods(level) if orc.K == 1 else [t]):
                assert digits_at_max(orc, level, tt, x[-1][1]) == expected_digits(orc, level, tt), (level, tt)
        return targets, np.stack(x)


_caches = {name: SchemeCache() for name in MAC_CHAINS}


def _env(name, oracle_mod):
    def make():
        e = Env(oracle_mod, name)
        return e.lib, e
    return _caches[name].get(make)[1]


@pytest.fixture
def edge(torch_cuda, oracle_mod):
    e = _env("edge", oracle_mod)
    assert [q.bit_length() for q in e.mods] == EDGE_BITS
    return e


@pytest.fixture
def wide(torch_cuda, oracle_mod):
    return _env("wide", oracle_mod)


def delete(lib, handles):
    for h in set(handles):
        lib.DeleteCiphertext(h)


def profiled(lib, fn):
    lib.OrionHipProfileReset()
    lib.OrionHipProfile(1)
    r = fn()
    lib.OrionHipProfile(0)
    p = lib.profile_read()
    return r, {k: p[k]["launches"] for k in p}


def beta_of(env, level):
    return len(digit_limbs(level, env.orc.K))


# ---- a. RotateNew and OrionHipRotateAdd under a max key --------------------------------------------
def check_rotate(env, x, level, amount):
    """RotateNew and OrionHipRotateAdd of every image of x by `amount` under its
    max key, against Oracle.rotate; returns the rotation's launch counts"""
    lib, orc = env.lib, env.orc
    g = env.g(amount)
    key = env.max_keys([g])[g]
    qs = np.array(env.mods[:level + 1], dtype=np.uint64)[:, None]
    ct, ca = lib.import_ciphertext(x, SCALE), lib.import_ciphertext(x, SCALE)

    def run():  # (a rotation runs when its result is read)
        r = lib.RotateNew(ct, amount)
        return r, lib.export_ciphertext(r)

    delete(lib, [run()[0]])  # (tables: first use)
    (r, got), prof = profiled(lib, run)
    lib.OrionHipRotateAdd(ca, amount)
    got_a = lib.export_ciphertext(ca)
    assert np.array_equal(lib.export_galois_key(g), key)  # still the planted key
    for b in range(x.shape[0]):
        ref = orc.rotate(x[b], g, key, level)
        assert np.array_equal(got[b], ref), ("rotate", level, b)
        assert np.array_equal(got_a[b], (x[b] + ref) % qs), ("rotate-add", level, b)
    delete(lib, [ct, ca, r])
    return prof


@pytest.mark.parametrize("level", [7, 4])
def test_rotate_max_key_edge(edge, level):
    """EDGE at level 7: beta = 4, every digit at t - 1; at level 4: beta = 3 and
    a last digit of one 54-bit prime, so 2 of 3 on the 60- and 61-bit targets
    (tests/test_planted_mac.py::test_digit_counts).  One image per limb."""
    assert beta_of(edge, level) == (4 if level == 7 else 3)
    targets, x = edge.images(level, np.random.default_rng(70 + level))
    assert len(targets) == level + 1 + edge.orc.K
    prof = check_rotate(edge, x, level, 3)
    assert prof.get("ks_mac", 0) >= 1, prof


def test_rotate_max_key_latency_routes(torch_cuda, oracle_mod):
    """N = 2^15, level 5, B = 2 (targets p_0 and q_0): the ks_mac_rows /
    ks_mac_full routes of test_latency_routes, the extension formed in the NTT
    prologue as in test_modup_planted_ntt_prologue"""
    lat = _env("lat", oracle_mod)
    orc = lat.orc
    rng = np.random.default_rng(75)
    x = np.stack([max_digit_ct(orc, 5, t, rand_poly(rng, lat.mods, list(range(6)), orc.N)) for t in (orc.L, 0)])
    for t, img in zip((orc.L, 0), x):
        assert digits_at_max(orc, 5, t, img[1]) == 3 == beta_of(lat, 5)
    prof = check_rotate(lat, x, 5, 7)
    assert prof.get("ntt_bext", 0) > 0 and prof.get("ks_mac", 0) >= 1, prof


def test_rotate_max_key_one_prime_gadget_wide(torch_cuda, oracle_mod, monkeypatch):
    """the K = 1, 16-limb N = 2^15 chain of test_one_prime_gadget_wide_fused_mac
    with its ORION_NTT_IFUSE_MAXR setting (ks_mac_full_kernel, beta = 16),
    B = 1: every digit at the maximum on every limb"""
    monkeypatch.setenv("ORION_NTT_IFUSE_MAXR", "1000")
    env = Env(oracle_mod, "wide16")
    try:
        level = 15
        assert beta_of(env, level) == 16
        targets, x = env.images(level, np.random.default_rng(76))
        assert x.shape[0] == 1
        prof = check_rotate(env, x, level, 1)
        assert prof.get("ks_mac", 0) >= 1, prof
    finally:
        env.lib.DeleteScheme()


# ---- b. rotate_hoisted under max keys for every amount ---------------------------------------------
AMOUNTS17 = list(range(1, 18))  # two chunks of ks_mac_hoisted


def check_hoisted(env, x, level):
    lib, orc = env.lib, env.orc
    gels = [env.g(k) for k in AMOUNTS17]
    keys = env.max_keys(gels)
    ct = lib.import_ciphertext(x, SCALE)
    delete(lib, lib.rotate_hoisted(ct, AMOUNTS17))  # (tables: first use)
    outs, prof = profiled(lib, lambda: lib.rotate_hoisted(ct, AMOUNTS17))
    assert len(outs) == len(AMOUNTS17)
    for k, g, h in zip(AMOUNTS17, gels, outs):
        got = lib.export_ciphertext(h)
        for b in range(x.shape[0]):
            assert np.array_equal(got[b], orc.rotate(x[b], g, keys[g], level)), (k, level, b)
        r = lib.RotateNew(ct, k)
        assert np.array_equal(lib.export_ciphertext(r), got), k
        lib.DeleteCiphertext(r)
    for g in gels:
        assert np.array_equal(lib.export_galois_key(g), keys[g])
    delete(lib, outs + [ct])
    return prof


def test_hoisted_max_keys_edge(edge):
    """EDGE level 7: beta = 4, the <4> instantiation exactly full"""
    assert beta_of(edge, 7) == 4
    _, x = edge.images(7, np.random.default_rng(80))
    prof = check_hoisted(edge, x, 7)
    assert prof["ks_mac"] == -(-len(AMOUNTS17) // MAXHOIST), prof


@pytest.mark.parametrize("level", [7, 8])
def test_hoisted_max_keys_wide(wide, level):
    """K = 1: beta = 8, the <8> instantiation exactly full (one launch per 16
    keys), and beta = 9, the grouped fallback past hoist::in_registers"""
    assert beta_of(wide, level) == level + 1
    _, x = wide.images(level, np.random.default_rng(81 + level))
    x = np.concatenate([x, x])  # (K = 1: one image attacks every limb; a second row of the grid)
    prof = check_hoisted(wide, x, level)
    if level == 7:
        assert prof["ks_mac"] == -(-len(AMOUNTS17) // MAXHOIST), prof
    else:
        assert prof.get("ks_mac", 0) >= 1, prof


# ---- c. rotate_sum: lt_giant_kernel at both reduction schemes' bounds ------------------------------
def sum_amounts(n, zero):
    """n rotating amounts over 8 keys (a repeated amount is a giant of its own), and the identity"""
    return ([0] if zero else []) + [1 + i % 8 for i in range(n)]


SUM_CASES = {7: [(25, True), (48, True), (64, False)],  # 5 terms per giant: a flush and a remainder, two exact fills,
             5: [(31, True), (60, False)]}              # the group limit; 4 per giant: a flush after 30, two fills


@pytest.mark.parametrize("layout", ["alone", 1, 5])
@pytest.mark.parametrize("level", [7, 5])
def test_rotate_sum_max_keys(edge, level, layout):
    """c0 = -P^-1, so that the P c0 addend is q - 1 on every Q limb; max keys
    meeting on M.  On M, level 7 (beta = 4): 4 products of (q - 1)^2 per
    mac_reduce on the 54-, 60- and 61-bit limbs, and 5 terms per giant in the
    small accumulator of the 40..52-bit limbs, 120 of 120 after 24 giants;
    level 5 (beta = 3): 4 terms per giant, 120 after 30.  "alone": every image
    as a launch of its own (IB = 1: 4 digits per chunk); 1 and 5: the
    per-target set that many times in one batch (IB = 4: 2 per chunk), 10, 50,
    8 + 1 and 40 + 1 images: a partial last group each (the oracle runs on the
    per-target images only)."""
    lib, orc = edge.lib, edge.orc
    beta = beta_of(edge, level)
    assert beta == (4 if level == 7 else 3) and 120 % (beta + 1) == 0
    targets, x = edge.images(level, "negpinv")
    gels8 = [edge.g(k) for k in range(1, 9)]
    keys = edge.max_keys(gels8)

    def make():
        memo = {}
        return {(n, z): sum_expected(orc, x, [edge.g(k) for k in sum_amounts(n, z)], keys, level, memo)
                for n, z in SUM_CASES[level]}

    refs = edge.cached(("sum", level), keys, make)
    T = len(targets)
    if layout == "alone":
        batches = [[b] for b in range(T)]
    else:
        rows = list(range(T)) * layout
        batches = [rows + ([0] if len(rows) % 4 == 0 else [])]
        assert len(batches[0]) % 4 != 0
    for n, z in SUM_CASES[level]:
        amounts = sum_amounts(n, z)
        assert n * (beta + 1) >= 120 and len(amounts) <= 64
        for rows in batches:
            ct = lib.import_ciphertext(x[rows], SCALE)
            h, prof = profiled(lib, lambda: lib.rotate_sum(ct, amounts))
            assert prof["lt_giant"] == 1 and prof.get("ks_mac", 0) == 0, prof
            got = lib.export_ciphertext(h)
            for i, b in enumerate(rows):
                assert np.array_equal(got[i], refs[n, z][b]), (level, n, z, layout, i, b)
            delete(lib, [ct, h])


# ---- d. MulRelinCiphertextNew under a planted relinearisation key ----------------------------------
@pytest.mark.parametrize("level", [7, 4])
def test_mul_relin_planted_key(edge, torch_cuda, level):
    """the relinearisation key's words q_m - 1 on M; b = (random, 1), so that
    d2 = a1 is the max_digit_ct row (ones_cts' trick, test_gpu_bext_planted.py)"""
    lib, orc = edge.lib, edge.orc
    if "rlk" not in edge.refs:
        rlk = max_key(lib.export_relin_key(), edge.mods, edge.M)
        plant_relin_key(lib, torch_cuda, rlk)
        edge.refs["rlk"] = rlk
    rlk = edge.refs["rlk"]
    assert np.array_equal(lib.export_relin_key(), rlk)
    rng = np.random.default_rng(90 + level)
    _, x = edge.images(level, rng)
    y = np.stack([np.stack([rand_poly(rng, edge.mods, list(range(level + 1)), orc.N),
                            np.ones((level + 1, orc.N), dtype=np.uint64)]) for _ in range(x.shape[0])])
    ca, cb = lib.import_ciphertext(x, SCALE), lib.import_ciphertext(y, SCALE)
    cm = lib.MulRelinCiphertextNew(ca, cb)
    got = lib.export_ciphertext(cm)
    assert lib.Rescale(cm) == cm
    got_s = lib.export_ciphertext(cm)
    for b in range(x.shape[0]):
        ref = orc.mul_relin(x[b], y[b], rlk, level)
        assert np.array_equal(got[b], ref), ("mul_relin", level, b)
        assert np.array_equal(got_s[b], orc.rescale(ref, level)), ("rescale", level, b)
    delete(lib, [ca, cb, cm])


# ---- e, f. EvaluateLinearTransform --------------------------------------------------------------------
LT_LEVEL = 7
LT_RATIO = 4.0  # LogBabyStepGiantStepRatio = 1


def lt_rotations(orc, idx, n1):
    split = [bsgs_split(d, orc.slots, n1) for d in idx]
    return sorted({b for _, b in split}), sorted({g for g, _ in split} - {0}), split


def planted_diagonal_blob(env, rng):
    """wire words of one QP diagonal: q_m - 1 on M, random residues elsewhere"""
    rows = {}
    for m in env.orc.qp_mods(LT_LEVEL):
        q = env.mods[m]
        r = rng.integers(0, q, env.orc.N, dtype=np.uint64)
        r[env.M] = mform(q - 1, q)
        rows[m] = r
    return qp_blob(env.orc, LT_LEVEL, rows)


def make_transform(env, which, variant):
    """variant "diag": "load" mode, planted diagonals, digit-0 baby keys;
    variant "keys": the scheme's own encoding of random diagonals, max baby
    keys.  Giants' keys are the scheme's own.  Returns (lt, idx, N1, pts, gkeys)."""
    lib, orc = env.lib, env.orc
    idx = LT_IDX[which]
    rng = np.random.default_rng(len(idx) + (variant == "keys"))
    if variant == "diag":
        lt = lib.GenerateLinearTransform(idx, [], LT_LEVEL, LT_RATIO, "load")
    else:
        diags = rng.uniform(-1, 1, (len(idx), lib.slots)).astype(np.float32)
        lt = lib.GenerateLinearTransform(idx, list(diags.reshape(-1)), LT_LEVEL, LT_RATIO, "none")
    n1 = lib.GetLinearTransformN1(lt)
    babies, giants, split = lt_rotations(orc, idx, n1)
    # by the plan's indices: no s = 0 baby, and the fullest giant holds N1 - 1 babies, all of them rotating
    assert 0 not in babies and len(babies) == n1 - 1
    assert max(sum(1 for g, _ in split if g == gi) for gi in {g for g, _ in split}) == n1 - 1
    gels = sorted(int(g) for g in lib.GetLinearTransformRotationKeys(lt) if g != 1)
    bg, gg = [env.g(b) for b in babies], [env.g(g) for g in giants]
    assert set(bg + gg) == set(gels) and not set(bg) & set(gg)
    gkeys = dict(env.own_keys(gg))
    gkeys.update(env.digit0_keys(bg) if variant == "diag" else env.max_keys(bg))
    assert all(lib.GetGaloisKeyLevel(g) == LT_LEVEL for g in gels)
    if variant == "diag":
        for d in idx:
            lib.LoadPlaintextDiagonal(planted_diagonal_blob(env, rng), lt, d)
    pts = [lib.export_lt_diagonal(lt, d, LT_LEVEL) for d in idx]
    if variant == "diag":
        for p in pts:
            for k, m in enumerate(orc.qp_mods(LT_LEVEL)):
                assert np.all(p[k][env.M] == env.mods[m] - 1)
    return lt, idx, n1, pts, gkeys


def check_transform(env, which, variant, layout):
    """"alone": every per-target image as a call of its own (one image per
    workgroup); 1 and 5: the per-target set that many times in one call, 10
    and 50 images (four images per workgroup, a partial last group; the
    oracle runs on the per-target images only)"""
    lib, orc = env.lib, env.orc
    assert beta_of(env, LT_LEVEL) == 4
    targets, x = env.images(LT_LEVEL, "zero" if variant == "diag" else np.random.default_rng(95))
    assert all(expected_digits(orc, LT_LEVEL, t) == 4 for t in targets)  # digit 0 among them
    lt, idx, n1, pts, gkeys = make_transform(env, which, variant)
    assert n1 == (8 if which == "lt8" else 16)
    try:
        refs = env.cached((which, variant), gkeys,
                          lambda: [orc.lt_bsgs(img, LT_LEVEL, idx, pts, n1, gkeys) for img in x])
        T = len(targets)
        batches = [[b] for b in range(T)] if layout == "alone" else [list(range(T)) * layout]
        assert layout == "alone" or len(batches[0]) % 4 != 0
        for rows in batches:
            ct = lib.import_ciphertext(x[rows], SCALE)
            y = lib.EvaluateLinearTransform(lt, ct)
            got = lib.export_ciphertext(y)
            assert lib.Rescale(y) == y
            got_s = lib.export_ciphertext(y)
            for i, b in enumerate(rows):
                assert np.array_equal(got[i], refs[b]), (which, variant, layout, i, b)
                assert np.array_equal(got_s[i], orc.rescale(refs[b], LT_LEVEL)), (which, variant, layout, i, b)
            delete(lib, [ct, y])
        for g, k in gkeys.items():
            assert np.array_equal(lib.export_galois_key(g), k)
    finally:
        lib.DeleteLinearTransform(lt)


@pytest.mark.parametrize("layout", ["alone", 1, 5])
@pytest.mark.parametrize("which", ["lt8", "lt16"])
def test_linear_transform_planted_diagonals(edge, which, layout):
    """e: c0 = 0 and baby keys of word 1 in digit 0, so every rotating baby is
    t - 1 in both components on the target limb, and diagonals of q_m - 1 on M:
    each of the fullest giant's N1 - 1 products is (t - 1)^2 there.  N1 = 8 runs
    the 8-slot kernels with 7 slots at the maximum, N1 = 16 the 16-slot kernels
    with 15: MacD on the 40/41/48-bit limbs, MacW + macw_reduce8 on 49..60,
    the 4-product MacAcc on 61."""
    check_transform(edge, which, "diag", layout)


@pytest.mark.parametrize("layout", ["alone", 1, 5])
@pytest.mark.parametrize("which", ["lt8", "lt16"])
def test_linear_transform_max_baby_keys(edge, which, layout):
    """f: max baby keys and the scheme's own diagonals: gadget_at's 4-product
    chunks (beta = 4) at their bound on M inside the fused kernel"""
    check_transform(edge, which, "keys", layout)
