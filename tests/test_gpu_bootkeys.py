"""Bootstrapping without the secret key (GPU): a scheme that never held the
secret builds the circuits (NewBootstrapper), imports the key owner's records
(OrionHipExportBootstrapKey / OrionHipImportBootstrapKey) and bootstraps to
the owner's output bit for bit.

Shapes of test_bootstrap_parity: N = 2^13, residual chain [60] + [40] * 5, P
[60, 60], logPs [61, 61], h = 192, batch 2.  Two slot counts on one scheme
(one shared bootstrapping context): n = N/2 (X^(N/2) plaintext, two EvalMods,
no trace) and n/8 (trace keys, the packed EvalMod).

The scheme is process-global, so the key owner runs first, once for the module
(fixture `owner`): everything the keyless schemes need from it is exported
before its DeleteScheme."""
import ctypes
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOGQ = [60] + [40] * 5  # the residual chain (test_gpu_parity.BTP_LOGQ)
LOGP = [60, 60]
LOGPS = [61, 61]
SCALE = 2.0 ** 40
KINDS = {"relin": 1, "d2s": 2, "s2d": 3, "galois": 4}
# test_bootstrap_functional's bars (max, mean) on the decrypted error at h = 192: full
# slots 2.5e-7 / 3e-8; a sparse slot count other than 64 gets its default 3e-7 / 5e-8
BARS = {"full": (2.5e-7, 3e-8), "sparse": (3e-7, 5e-8)}


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _scheme(seed, logq=LOGQ, secret=True):
    from orion_amd.backend import HipLibrary
    lib = HipLibrary().new_scheme(13, logq, LOGP, 40, h=192, seed=seed)
    if secret:
        lib.GenerateSecretKey()
        lib.GeneratePublicKey()
        lib.GenerateRelinearizationKey()
    return lib


def _values(n, ns):
    vals = np.random.default_rng(900 + ns).uniform(-1, 1, (2, n)).astype(np.float32)
    vals[:, ns:] = 0
    return vals


def _records(lib, ns):
    return [lib.export_bootstrap_key(ns, i) for i in range(len(lib.bootstrap_key_info(ns)))]


@pytest.fixture(scope="module")
def owner(torch_cuda):
    """The key owner's side, run once: a record of another chain first, then
    scheme A -- PrepareKeys (no warm-up Bootstrap), one Bootstrap per slot
    count, every export -- and its DeleteScheme."""
    torch = torch_cuda
    o = {}
    # a record made for another residual chain ([60] + [40] * 4)
    other = _scheme(23, [60] + [40] * 4)
    other.NewBootstrapper(LOGPS, other.N // 2 // 8)
    o["other_chain_record"] = other.export_bootstrap_key(other.N // 2 // 8, 0)
    other.DeleteScheme()

    lib = _scheme(21)
    n = lib.N // 2
    o["n"], o["slot_counts"] = n, (n, n // 8)
    for ns in o["slot_counts"]:
        lib.NewBootstrapper(LOGPS, ns)
    o["missing_before_prepare"] = {ns: lib.bootstrap_missing_keys(ns) for ns in o["slot_counts"]}
    t0 = time.perf_counter()
    # (returned count, records held right then: the second circuit's keys join the shared context later)
    # the sparse circuit first, and its records as they are then: a Galois element that the
    # full circuit uses at a higher level is still held at the sparse circuit's level
    o["prepared_count"] = {n // 8: (lib.bootstrap_prepare_keys(n // 8), len(lib.bootstrap_key_info(n // 8)))}
    o["prepare_s"] = time.perf_counter() - t0
    o["sparse_early_info"] = lib.bootstrap_key_info(n // 8)
    o["sparse_early_records"] = _records(lib, n // 8)
    t0 = time.perf_counter()
    o["prepared_count"][n] = (lib.bootstrap_prepare_keys(n), len(lib.bootstrap_key_info(n)))
    o["prepare_s"] += time.perf_counter() - t0
    o["missing_after_prepare"] = {ns: lib.bootstrap_missing_keys(ns) for ns in o["slot_counts"]}
    o["info_prepared"] = {ns: lib.bootstrap_key_info(ns) for ns in o["slot_counts"]}
    o["x"], o["out"], o["out_level"], o["out_scale"], o["err"], o["info_after"] = {}, {}, {}, {}, {}, {}
    for ns in o["slot_counts"]:
        vals = _values(n, ns)
        ct = lib.Encrypt(lib.encode_batch(vals, 0, 1 << 40))
        out = lib.Bootstrap(ct, ns)
        # (every slot count's records, after each Bootstrap: nothing made, nothing replaced)
        o["info_after"][ns] = {m: lib.bootstrap_key_info(m) for m in o["slot_counts"]}
        o["x"][ns], o["out"][ns] = lib.export_ciphertext(ct), lib.export_ciphertext(out)
        o["out_level"][ns], o["out_scale"][ns] = lib.GetCiphertextLevel(out), lib.GetCiphertextScaleF(out)
        exp = np.tile(vals[:, :ns], (1, n // ns)).astype(np.float64)
        o["err"][ns] = np.abs(lib.decode_f64(lib.Decrypt(out)) - exp)
    nb = int(lib.KeyBundleBytes(0))
    o["bundle"] = torch.empty(nb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.lib.ExportKeyBundle(o["bundle"].data_ptr(), 0) == 0
    t0 = time.perf_counter()
    o["records"] = {ns: _records(lib, ns) for ns in o["slot_counts"]}
    o["export_s"] = time.perf_counter() - t0
    for ns in o["slot_counts"]:
        nbytes = sum(r.numel() for r in o["records"][ns])
        print("bootstrap keys N=2^13 slots=%d: %d records, %d bytes" % (ns, len(o["records"][ns]), nbytes))
    print("prepare %.3f s, export %.3f s" % (o["prepare_s"], o["export_s"]))
    print("keys missing before PrepareKeys:", o["missing_before_prepare"], "records held after each PrepareKeys:",
          o["prepared_count"], "sparse circuit's records before the full circuit's: %d bytes"
          % sum(r.numel() for r in o["sparse_early_records"]))
    lib.DeleteScheme()
    return o


def _keyless(owner, import_keys):
    """Scheme B: A's parameters, another seed, A's key bundle without the
    secret, both circuits; with import_keys, A's records -- the sparse circuit's
    first (as they were before the full circuit's keys were made, then as they
    ended), so an element both circuits use arrives at its lower level first."""
    lib = _scheme(22, secret=False)
    assert lib.lib.ImportKeyBundle(owner["bundle"].data_ptr(), owner["bundle"].numel()) == 0
    for ns in owner["slot_counts"]:
        lib.NewBootstrapper(LOGPS, ns)
    if import_keys:
        _import_all(lib, owner)
    return lib


def _import_all(lib, owner):
    full, sparse = owner["slot_counts"]
    for ns, recs in ((sparse, owner["sparse_early_records"]), (sparse, owner["records"][sparse]),
                     (full, owner["records"][full])):
        for r in recs:
            lib.import_bootstrap_key(ns, r)


def _check_bootstrap(lib, owner, ns):
    ct = lib.import_ciphertext(owner["x"][ns], SCALE)
    out = lib.Bootstrap(ct, ns)
    assert lib.GetCiphertextLevel(out) == owner["out_level"][ns] == len(LOGQ) - 1
    assert lib.GetCiphertextScaleF(out) == owner["out_scale"][ns]
    assert np.array_equal(lib.export_ciphertext(out), owner["out"][ns]), ns
    lib.DeleteCiphertext(out)
    return ct


def test_keyless_bootstrap_equals_owner(owner):
    """Scheme B never holds the secret; with A's records its Bootstrap output
    (words, level, scale) is A's exactly, for both slot counts.  A's own
    outputs decrypt within test_bootstrap_functional's bars."""
    n, full, sparse = owner["n"], owner["slot_counts"][0], owner["slot_counts"][1]
    assert all(v > 0 for v in owner["missing_before_prepare"].values())
    assert all(v == 0 for v in owner["missing_after_prepare"].values())
    for ns, bar in ((full, BARS["full"]), (sparse, BARS["sparse"])):
        err = owner["err"][ns]
        print("owner bootstrap ns=%d err max %.3g mean %.3g" % (ns, err.max(), err.mean()))
        assert err.max() < bar[0] and err.mean() < bar[1], (ns, err.max(), err.mean())
    lib = _keyless(owner, import_keys=False)
    try:
        missing = {ns: lib.bootstrap_missing_keys(ns) for ns in owner["slot_counts"]}
        assert all(v > 0 for v in missing.values()), missing
        t0 = time.perf_counter()
        _import_all(lib, owner)
        print("import %.3f s" % (time.perf_counter() - t0))
        assert {ns: lib.bootstrap_missing_keys(ns) for ns in owner["slot_counts"]} == {full: 0, sparse: 0}
        # a shared element came at the sparse circuit's level first: the higher level stays
        early = {r[1]: r[2] for r in owner["sparse_early_info"] if r[0] == KINDS["galois"]}
        final = {r[1]: r[2] for r in owner["info_prepared"][full] if r[0] == KINDS["galois"]}
        raised = {g: (early[g], final[g]) for g in early if final[g] > early[g]}
        print("elements the full circuit raised above the sparse circuit's level:", raised)
        assert raised and all(final[g] >= early[g] for g in early)
        assert lib.bootstrap_key_info(full) == owner["info_prepared"][full]
        assert lib.bootstrap_key_info(sparse) == owner["info_prepared"][sparse]
        cts = [_check_bootstrap(lib, owner, ns) for ns in owner["slot_counts"]]
        with pytest.raises(RuntimeError, match="secret key"):
            lib.Decrypt(cts[0])
        with pytest.raises(RuntimeError, match="no secret key"):
            lib.export_secret_key()
    finally:
        lib.DeleteScheme()
    assert n == full


def test_need_list_is_the_truth(owner):
    """Prepared keys are exactly the keys the circuits use: a Bootstrap of
    either slot count makes and replaces nothing, and a scheme of the same seed
    warmed up lazily (two Bootstraps per slot count, no PrepareKeys) ends with
    the same Galois elements, none at a higher level than the prepared one."""
    full, sparse = owner["slot_counts"]
    for ns in owner["slot_counts"]:
        assert owner["prepared_count"][ns][0] == owner["prepared_count"][ns][1] > 3
        assert owner["info_after"][ns] == owner["info_prepared"], ns
        # record order: relin, d2s, s2d, then the Galois keys by ascending element
        info = owner["info_prepared"][ns]
        assert [r[0] for r in info[:3]] == [1, 2, 3] and all(r[0] == 4 for r in info[3:])
        gels = [r[1] for r in info[3:]]
        assert gels == sorted(set(gels))
    lib = _scheme(21)
    try:
        n = lib.N // 2
        for ns in owner["slot_counts"]:
            lib.NewBootstrapper(LOGPS, ns)
        for ns in owner["slot_counts"]:
            ct = lib.Encrypt(lib.encode_batch(_values(n, ns), 0, 1 << 40))
            for _ in range(2):
                lib.DeleteCiphertext(lib.Bootstrap(ct, ns))
        for ns in owner["slot_counts"]:
            assert lib.bootstrap_missing_keys(ns) == 0
            warmed = {r[1]: r[2] for r in lib.bootstrap_key_info(ns) if r[0] == KINDS["galois"]}
            prepared = {r[1]: r[2] for r in owner["info_prepared"][ns] if r[0] == KINDS["galois"]}
            assert sorted(warmed) == sorted(prepared)
            higher = {g: (prepared[g], warmed[g]) for g in prepared if prepared[g] != warmed[g]}
            print("ns=%d: %d galois keys, prepared above warmed: %s" % (ns, len(prepared), higher))
            assert all(prepared[g] >= warmed[g] for g in prepared), higher
    finally:
        lib.DeleteScheme()


def test_refusals_leave_the_bootstrapper_usable(owner, torch_cuda):
    """Every refused call raises RuntimeError naming its cause and changes
    nothing: afterwards a valid import and Bootstrap succeed."""
    torch = torch_cuda
    full, sparse = owner["slot_counts"]
    lib = _keyless(owner, import_keys=False)
    try:
        x = lib.import_ciphertext(owner["x"][full], SCALE)
        need = lib.bootstrap_missing_keys(full)
        with pytest.raises(RuntimeError, match=r"lacks %d of its %d evaluation keys.*relin key" % (need, need)):
            lib.Bootstrap(x, full)
        with pytest.raises(RuntimeError, match="needs the secret key"):
            lib.bootstrap_prepare_keys(full)
        before = {ns: lib.bootstrap_key_info(ns) for ns in owner["slot_counts"]}
        assert before == {full: [], sparse: []}
        recs = owner["records"][full]
        kinds = [r[0] for r in owner["info_prepared"][full]]
        d2s = recs[kinds.index(KINDS["d2s"])]
        bad_magic = recs[0].clone()
        bad_magic[0] ^= 0xFF
        for pattern, call in (
                ("bad magic", lambda: lib.import_bootstrap_key(full, bad_magic)),
                ("another bootstrapping chain", lambda: lib.import_bootstrap_key(full, owner["other_chain_record"])),
                ("belongs to the circuit for %d slots, not %d" % (full, sparse),
                 lambda: lib.import_bootstrap_key(sparse, d2s)),
                ("truncated", lambda: lib.import_bootstrap_key(full, recs[0][:-1])),
                ("shorter than its header", lambda: lib.import_bootstrap_key(full, recs[0][:255])),
                ("no bootstrapper found for slot count: 64", lambda: lib.import_bootstrap_key(64, recs[0])),
                ("no bootstrapper found for slot count: 64", lambda: lib.bootstrap_key_info(64)),
                ("no bootstrapper found for slot count: 64", lambda: lib.bootstrap_missing_keys(64)),
                ("record 0 out of range: 0 records", lambda: lib.export_bootstrap_key(full, 0))):
            with pytest.raises(RuntimeError, match=pattern):
                call()
            assert {ns: lib.bootstrap_key_info(ns) for ns in owner["slot_counts"]} == before, pattern
        # the keys of the first Bootstrap's error message: the first record is the relinearisation key
        lib.import_bootstrap_key(full, recs[0])
        with pytest.raises(RuntimeError, match=r"lacks %d of its %d evaluation keys.*d2s key" % (need - 1, need)):
            lib.Bootstrap(x, full)
        _import_all(lib, owner)
        count = len(lib.bootstrap_key_info(full))
        with pytest.raises(RuntimeError, match="record %d out of range: %d records" % (count, count)):
            lib.export_bootstrap_key(full, count)
        # no new call inside a graph capture (raw entries: the wrappers' stream
        # waits would themselves disturb the capture)
        buf = torch.empty(int(lib.OrionHipBootstrapKeyBytes(full, 0)), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        info4 = (ctypes.c_ulong * 4)()
        lib.OrionHipGraphBegin()
        clone = None
        try:
            for name, args in (("OrionHipBootstrapPrepareKeys", (full,)), ("OrionHipBootstrapMissingKeys", (full,)),
                               ("OrionHipBootstrapKeyCount", (full,)), ("OrionHipBootstrapKeyBytes", (full, 0)),
                               ("OrionHipBootstrapKeyInfo", (full, 0, info4)),
                               ("OrionHipExportBootstrapKey", (full, 0, buf.data_ptr())),
                               ("OrionHipImportBootstrapKey", (full, buf.data_ptr(), buf.numel()))):
                with pytest.raises(RuntimeError, match=name + " is not allowed while capturing"):
                    getattr(lib, name)(*args)
            clone = lib.CloneCiphertext(x)  # (the capture records something)
        finally:
            gid = lib.OrionHipGraphEnd()
        lib.OrionHipGraphDestroy(gid)
        lib.DeleteCiphertext(clone)
        # the library is usable afterwards: both circuits give the owner's outputs
        for ns in owner["slot_counts"]:
            _check_bootstrap(lib, owner, ns)
    finally:
        lib.DeleteScheme()


def test_delete_bootstrappers_drops_imported_keys(owner):
    full, sparse = owner["slot_counts"]
    lib = _keyless(owner, import_keys=True)
    try:
        x = lib.import_ciphertext(owner["x"][sparse], SCALE)
        assert len(lib.bootstrap_key_info(sparse)) > 3
        lib.DeleteBootstrappers()
        with pytest.raises(RuntimeError, match="no bootstrapper found"):
            lib.Bootstrap(x, sparse)
        for ns in owner["slot_counts"]:
            with pytest.raises(RuntimeError, match="no bootstrapper found"):
                lib.OrionHipBootstrapKeyCount(ns)
        # a new bootstrapper starts with no keys: the imported ones are gone
        lib.NewBootstrapper(LOGPS, sparse)
        assert lib.bootstrap_key_info(sparse) == []
    finally:
        lib.DeleteScheme()
