"""The encoder (enc_load_kernel, the special iFFT fft_lds_kernel /
fft_outer_kernel<G>, enc_crt_kernel; csrc/encoder.hip) on planted inputs.

A. An image whose every slot is the same real c encodes to the constant
   polynomial X = rule(fl(c * scale)): the iFFT's sums double, its differences
   are zero and n c (1/n) is exact, so the plaintext's NTT rows are the
   constant rows X mod q_j.  (c, scale) on every edge of the fixed-point rule
   (helpers.encode_planted_cases) against exact integers (helpers.fixed_point_rule).
B. Encode and decode bit for bit against the oracle at every FFT split G =
   log2(slots) - 12 that no other direct test reaches (G = 1, 2 Standard; G =
   2, 3 ConjugateInvariant).
C. The diagonals GenerateLinearTransform encodes (rolled by the giant step, at
   scale q_level, over Q and P) against the oracle's own encoding.
D. Decode and encode against the canonical embedding evaluated directly in
   extended precision (helpers.canonical_slots).
E. A scale that is not finite and positive is refused on the host.

The CPU twins of A and D, on the oracle, are in tests/test_oracle.py."""
import ctypes

import numpy as np
import pytest

from tests.helpers import (EMBED_TOL, SMALL, SPLIT_CHAIN, SchemeCache, bsgs_split, canonical_slots, centred_coeffs,
                           constant_rows, embedding_plaintext, embedding_slots, encode_planted_cases, fixed_point_rule,
                           host_scale, plant_runs, planted_batches, split_images)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


_small_cache = {False: SchemeCache(), True: SchemeCache()}


def _small(oracle_mod, ci):
    """SMALL (Standard) or the ConjugateInvariant chain of test_gpu_ci.py, N = 2^13, no keys"""

    def make():
        from orion_amd.backend import HipLibrary
        p = SMALL
        lib = HipLibrary().new_scheme(p["logn"], p["logq"], p["logp"], 40, h=192, seed=77,
                                      ringtype="ConjugateInvariant" if ci else "standard")
        orc = oracle_mod.Oracle(p["logn"], lib.moduli(), len(p["logq"]), len(p["logp"]), ci=ci)
        assert lib.N == orc.N and lib.slots == orc.slots
        return lib, orc

    return _small_cache[ci].get(make)


# ---- A ----------------------------------------------------------------------
@pytest.mark.parametrize("ci", [False, True])
def test_encode_planted_fixed_point(torch_cuda, oracle_mod, ci):
    """Every planted (c, scale), both signs of c in one batch (blockIdx.y > 0),
    at level 5 through EncodeBatchDevice (a free float64 scale); the cases with
    an integer scale below 2^64 also through Encode and EncodeBatch (unsigned
    long).  The exported rows == constant_rows of the Python rule, and the
    oracle's encode gives the same rows (a failure names the side that is wrong)."""
    torch = torch_cuda
    lib, orc = _small(oracle_mod, ci)
    level = 5
    qs, mods = orc.moduli[:level + 1], list(range(level + 1))
    cases = encode_planted_cases(orc.moduli, oracle_mod.gen_moduli(14, [60], [])[0])
    nhost = 0
    for scale, imgs in planted_batches(cases).items():
        cs = np.array([c for _, c in imgs], dtype=np.float32)
        vals = np.repeat(cs[:, None], orc.slots, axis=1)
        exp = constant_rows([fixed_point_rule(c, scale) for c in cs], qs, orc.N)
        for b, (nm, c) in enumerate(imgs):
            ref = orc.encode(vals[b].astype(np.float64), scale, mods)
            assert np.array_equal(ref, exp[b]), ("oracle", nm, c, scale, ref[:, :2], exp[b][:, 0])
        got = {}  # path -> (exported rows, the images they are)
        pt = lib.encode_batch_device(torch.from_numpy(vals).cuda(), level, scale)
        got["EncodeBatchDevice"] = (lib.export_plaintext(pt), list(range(len(imgs))))
        lib.DeletePlaintext(pt)
        if host_scale(scale):
            nhost += 1
            pt = lib.encode_batch(vals, level, int(scale))
            got["EncodeBatch"] = (lib.export_plaintext(pt), list(range(len(imgs))))
            lib.DeletePlaintext(pt)
            pt = lib.Encode(list(vals[1]), level, int(scale))  # the negative sign
            got["Encode"] = (lib.export_plaintext(pt), [1])
            lib.DeletePlaintext(pt)
        for path, (rows, which) in got.items():
            assert rows.shape == exp[which].shape
            for r, b in zip(rows, which):
                nm, c = imgs[b]
                bad = np.argwhere(r != exp[b])
                assert bad.size == 0, ("GPU", path, nm, float(c), scale, [int(r[j, bad[0, 1]]) for j in mods],
                                       [int(x) for x in exp[b][:, 0]], len(bad))
    assert nhost >= 20


# ---- B ----------------------------------------------------------------------
# (ring logN, ConjugateInvariant): G = log2(slots) - 12.  Standard 2^13 (G = 0)
# has test_encode_parity, test_encode_batch_and_device_parity and
# test_decode_parity, Standard 2^16 (G = 3) test_n16_ops_parity
# (test_gpu_parity.py), CI 2^13 (G = 1) test_ci_encode_decode_parity
# (test_gpu_ci.py); the four below had none
SPLITS = [(14, False), (15, False), (14, True), (15, True)]


def _split_scheme(oracle_mod, logn, ci):
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(logn, SPLIT_CHAIN["logq"], SPLIT_CHAIN["logp"], 40,
                                  ringtype="ConjugateInvariant" if ci else "standard")
    orc = oracle_mod.Oracle(logn, lib.moduli(), 3, 1, ci=ci)
    assert lib.N == orc.N == 1 << logn and lib.slots == orc.slots
    return lib, orc


def _encode_split(torch, lib, orc, nvals, scale, level=2):
    """(images, exported rows) of one 3-image batch of nvals slots each; a
    scale past unsigned long goes through the device call's float64 scale"""
    vals = split_images(orc.slots, nvals, 1000 + nvals % 97)
    if scale >> 64:
        pt = lib.encode_batch_device(torch.from_numpy(vals).cuda(), level, float(scale))
    else:
        pt = lib.encode_batch(vals, level, scale)
    rows = lib.export_plaintext(pt)
    lib.DeletePlaintext(pt)
    return vals, rows


@pytest.mark.parametrize("logn,ci", SPLITS)
def test_encode_parity_every_split(torch_cuda, oracle_mod, logn, ci):
    """Batches of 3 images of slots - 5, 1 and slots values (enc_load_kernel's
    zero padding), +-4 planted at slots 0, 1, slots/2 and nvals - 1, at scales
    2^40 and 2^70 (the one-word and the exact path of enc_crt_kernel), bit for
    bit against the oracle's encode."""
    lib, orc = _split_scheme(oracle_mod, logn, ci)
    for nvals in (orc.slots - 5, 1, orc.slots):
        for scale in (1 << 40, 1 << 70):
            vals, rows = _encode_split(torch_cuda, lib, orc, nvals, scale)
            for b in range(3):
                ref = orc.encode(vals[b].astype(np.float64), float(scale), [0, 1, 2])
                assert np.array_equal(rows[b], ref), (nvals, scale, b)
    lib.DeleteScheme()


@pytest.mark.parametrize("logn,ci", SPLITS)
def test_decode_parity_every_split(torch_cuda, oracle_mod, logn, ci):
    """decode_f64 of three imported level-1 plaintexts (random residues, the
    same with constant runs of 0, 1 and q - 1 planted, all zeros) bit for bit
    against the oracle's decode; the zero image decodes to exact zeros."""
    lib, orc = _split_scheme(oracle_mod, logn, ci)
    rng = np.random.default_rng(70 + logn)
    rows = np.stack([np.stack([rng.integers(0, orc.moduli[j], orc.N, dtype=np.uint64) for j in range(2)])
                     for _ in range(3)])
    plant_runs(rows[1], orc.moduli)
    rows[2] = 0
    pt = lib.import_plaintext(rows, 2.0 ** 40)
    got = lib.decode_f64(pt)
    assert got.shape == (3, orc.slots)
    for b in range(3):
        assert np.array_equal(got[b], orc.decode(rows[b], 1, 2.0 ** 40)), b
    assert not got[2].any()
    lib.DeleteScheme()


# ---- C ----------------------------------------------------------------------
@pytest.mark.parametrize("ci", [False, True])
def test_linear_transform_diagonals_match_oracle_encoding(torch_cuda, oracle_mod, ci):
    """GenerateLinearTransform at level 4 (ratio arguments 2.0 and 4.0: log
    ratios 0 and 1) and level 0: N1 == the oracle's, and every stored diagonal
    == the oracle's encoding of the diagonal rolled right by its giant step, at
    scale float(q_level), over the Q limbs and the P limbs.  Uniform diagonals,
    one of magnitude about 1000 (at level 0, q_0 ~ 2^55, its coefficients pass
    2^64: the exact path on every limb), one all zero; indices that wrap
    (-3, slots + 2).  No key, no evaluation."""
    lib, orc = _small(oracle_mod, ci)
    slots = orc.slots
    idx = [0, 1, 17, 64, 65, slots - 1, -3, slots + 2]
    rng = np.random.default_rng(31 + ci)
    diags = rng.uniform(-1, 1, (len(idx), slots)).astype(np.float32)
    diags[2] += 1000  # coefficient 0 is the mean of the slots: 1000 q_0 > 2^64
    diags[4] = 0
    for level, ratio in ((4, 2.0), (4, 4.0), (0, 2.0)):
        lt = lib.GenerateLinearTransform(idx, list(diags.reshape(-1)), level, ratio, "none")
        n1 = lib.GetLinearTransformN1(lt)
        assert n1 == orc.find_best_bsgs_n1(idx, int(np.log(ratio))), (level, ratio)
        for i, d in enumerate(idx):
            giant, _ = bsgs_split(d, slots, n1)
            ref = orc.encode(np.roll(diags[i].astype(np.float64), giant), float(orc.moduli[level]), orc.qp_mods(level))
            got = lib.export_lt_diagonal(lt, d, level)
            assert got.shape == ref.shape == (level + 1 + orc.K, orc.N)
            assert np.array_equal(got, ref), (level, ratio, d, giant, np.argwhere(got != ref)[:4])
        if level == 0:  # the large diagonal's coefficient 0 took the exact path
            assert diags[2].astype(np.float64).mean() * float(orc.moduli[0]) > 2.0 ** 64
        lib.DeleteLinearTransform(lt)


# ---- D ----------------------------------------------------------------------
@pytest.mark.parametrize("logn,ci", [(13, False), (13, True), (15, False), (15, True)])
def test_decode_matches_canonical_embedding(torch_cuda, oracle_mod, logn, ci):
    """decode_f64 of the plaintext of signed coefficients uniform in +-2^45 at
    scale 2^40 (the CPU twin's, tests/test_oracle.py) against the embedding
    evaluated directly in extended precision, <= EMBED_TOL."""
    lib, orc = _split_scheme(oracle_mod, logn, ci)
    m, rows = embedding_plaintext(orc, 500 + logn)
    js = embedding_slots(orc.slots, np.random.default_rng(logn))
    exp = canonical_slots(m, js, ci) / np.longdouble(2.0 ** 40)
    got = lib.decode_f64(lib.import_plaintext(rows, 2.0 ** 40))[0]
    dev = float(np.abs(got[js].astype(np.longdouble) - exp).max())
    print(f"logn {logn} ci {ci}: max |slot| {float(np.abs(exp).max()):.3g}, deviation {dev:.3g}")
    assert dev <= EMBED_TOL, dev
    lib.DeleteScheme()


@pytest.mark.parametrize("ci", [False, True])
def test_encode_matches_canonical_embedding(torch_cuda, oracle_mod, ci):
    """The images of the split tests at N = 2^13, scale 2^40: the exported rows,
    inverse-NTT-ed and centred, are integer coefficients whose embedding at the
    checked slots is the float32 input (0 past nvals).  Bound: each coefficient
    is rounded by at most 1/2 and each slot sums N of them with weights of
    magnitude at most 1, N (1/2) / scale = 3.7e-9, plus the evaluation's 1e-10
    (EMBED_TOL; the iFFT's own float64 error, about 1e-15 per slot, is far below)."""
    logn, scale = 13, 2.0 ** 40
    lib, orc = _split_scheme(oracle_mod, logn, ci)
    vals, rows = _encode_split(torch_cuda, lib, orc, orc.slots - 5, 1 << 40)
    js = embedding_slots(orc.slots, np.random.default_rng(logn))
    bound = orc.N * 0.5 / scale + EMBED_TOL
    for b in range(3):
        m = centred_coeffs(orc, rows[b, 0])
        got = canonical_slots(m, js, ci) / np.longdouble(scale)
        exp = np.array([vals[b, j] if j < vals.shape[1] else 0.0 for j in js], dtype=np.longdouble)
        dev = float(np.abs(got - exp).max())
        print(f"ci {ci} image {b}: deviation {dev:.3g}, bound {bound:.3g}")
        assert dev <= bound, (b, dev)
    lib.DeleteScheme()


# ---- E ----------------------------------------------------------------------
def test_encode_refuses_a_bad_scale(torch_cuda, oracle_mod):
    """Encode, EncodeBatch (scale 0) and EncodeBatchDevice (0, -1, inf, nan):
    "scale must be finite and positive", handle -1, nothing launched, and the
    scheme encodes as before afterwards."""
    torch = torch_cuda
    lib, orc = _small(oracle_mod, False)
    vals = np.ones((2, 16), dtype=np.float32)
    dv = torch.from_numpy(vals).cuda()
    fp = vals.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    live = lib.GetLivePlaintexts()

    def refused(h):
        assert h == -1
        assert lib.lib.OrionHipLastError().decode() == "scale must be finite and positive"
        lib.lib.OrionHipClearError()

    refused(lib.lib.Encode(fp, 16, 3, 0))
    refused(lib.lib.EncodeBatch(fp, 16, 2, 3, 0))
    for s in (0.0, -1.0, float("inf"), float("nan"), -float("inf")):
        refused(lib.lib.EncodeBatchDevice(dv.data_ptr(), 16, 2, 3, s))
        with pytest.raises(RuntimeError, match="scale must be finite and positive"):
            lib.encode_batch_device(dv, 3, s)
    with pytest.raises(RuntimeError, match="scale must be finite and positive"):
        lib.Encode(list(vals[0]), 3, 0)
    with pytest.raises(RuntimeError, match="scale must be finite and positive"):
        lib.encode_batch(vals, 3, 0)
    assert lib.GetLivePlaintexts() == live
    pt = lib.encode_batch(vals, 3, 1 << 40)
    assert np.array_equal(lib.export_plaintext(pt)[1], orc.encode(vals[1].astype(np.float64), 2.0 ** 40, [0, 1, 2, 3]))
    lib.DeletePlaintext(pt)
