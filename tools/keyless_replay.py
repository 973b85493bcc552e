"""GPU: a model that bootstraps, served without the secret key.

The key owner compiles the op stream (default: resnet20_n13), prepares and
exports the bootstrapping keys record by record, runs its own forward pass and
exports the scheme's key bundle without the secret.  A fresh scheme (another
seed, no key generation) compiles with gen_keys=False, imports the bundle and
the records, and forwards the owner's input ciphertext; its output words are
compared bit for bit with the owner's.  One JSON line: record counts and bytes
per slot count, and the seconds PrepareKeys, export and import take."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orion_amd.replay import OrionStream  # noqa: E402


def main():
    import torch
    name = os.environ.get("WORKLOAD", "resnet20_n13")
    res = {"workload": name}
    st = OrionStream(name, seed=3)
    st.keygen()
    st.compile()
    lib = st.lib
    counts = st.bootstrap_slot_counts()
    res["needed_before_prepare"] = {ns: lib.bootstrap_missing_keys(ns) for ns in counts}
    t0 = time.perf_counter()
    for ns in counts:
        lib.bootstrap_prepare_keys(ns)
    res["prepare_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    records = st.export_bootstrap_keys()  # (PrepareKeys again: nothing left to make)
    lib.OrionHipSynchronize()
    res["export_s"] = round(time.perf_counter() - t0, 3)
    res["records"] = {ns: len(r) for ns, r in records.items()}
    res["record_bytes"] = {ns: int(sum(t.numel() for t in r)) for ns, r in records.items()}
    info = {ns: lib.bootstrap_key_info(ns) for ns in counts}
    ct = st.encrypt_batch(st.reference_input())
    x, scale = lib.export_ciphertext(ct), lib.GetCiphertextScaleF(ct)
    lib.DeleteCiphertext(st.forward(lib.CloneCiphertext(ct)))  # the scheme's own rotation keys, at their final levels
    res["bootstrap_keys_unchanged_by_forward"] = info == {ns: lib.bootstrap_key_info(ns) for ns in counts}
    out = st.forward(lib.CloneCiphertext(ct))
    want, want_scale = lib.export_ciphertext(out), lib.GetCiphertextScaleF(out)
    logits = st.decrypt_output(out)[0]
    exp = st.arrays["expected_output"].reshape(-1)
    res["owner_mae_vs_cleartext"] = float(np.abs(logits - exp).mean())
    bundle = torch.empty(int(lib.KeyBundleBytes(0)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if lib.lib.ExportKeyBundle(bundle.data_ptr(), 0) != 0:
        raise RuntimeError(lib.lib.OrionHipLastError().decode())
    res["scheme_bundle_bytes"] = bundle.numel()
    lib.DeleteScheme()

    srv = OrionStream(name, seed=4)  # no keygen(): this scheme never holds a secret
    lib = srv.lib
    lib.NewEncoder()
    lib.NewPolynomialEvaluator()
    lib.NewLinearTransformEvaluator()
    srv.compile(gen_keys=False)
    if lib.lib.ImportKeyBundle(bundle.data_ptr(), bundle.numel()) != 0:
        raise RuntimeError(lib.lib.OrionHipLastError().decode())
    res["server_missing_before_import"] = {ns: lib.bootstrap_missing_keys(ns) for ns in counts}
    t0 = time.perf_counter()
    srv.import_bootstrap_keys(records)
    lib.OrionHipSynchronize()
    res["import_s"] = round(time.perf_counter() - t0, 3)
    try:
        lib.export_secret_key()
        res["server_has_secret"] = True
    except RuntimeError:
        res["server_has_secret"] = False
    got_h = srv.forward(lib.import_ciphertext(x, scale))
    got = lib.export_ciphertext(got_h)
    res["bit_identical"] = bool(got.shape == want.shape and np.array_equal(got, want)
                                and lib.GetCiphertextScaleF(got_h) == want_scale)
    res["bootstraps"] = srv.forward_op_counts().get("Bootstrap", 0)
    print(json.dumps(res), flush=True)
    del records, bundle
    return 0 if res["bit_identical"] and not res["server_has_secret"] else 1


if __name__ == "__main__":
    sys.exit(main())
