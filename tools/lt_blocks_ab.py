"""A/B of the blocked linear transform against the op-by-op loop it replaces.

Two layers, each at batch 1 and 8: the first 4 x 4 convolution of the recorded
ResNet-20 stream at N = 2^13 (its own transforms and level, random input
residues) and the synthetic 2 x 3 layer of tests/test_gpu_ltblocks.py.  For
each, the profiled kernel time (OrionHipProfile: HIP events around every
launch, summed over the kernel families) of
  loop:    R C EvaluateLinearTransform, the AddCiphertextNew between them and R
           RescaleNew, as the frontend issues them (the unchanged path), and
  blocked: one OrionHipEvaluateLinearTransformBlocks call with rescale,
20 timed repetitions after 3 warm ones, on the same build and handles.

usage: python tools/lt_blocks_ab.py [--reps 20] [--warm 3] > profiles/NAME.txt
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orion_amd.backend import HipLibrary  # noqa: E402
from orion_amd.replay import OrionStream, block_groups  # noqa: E402

BIG = [0, 1, 2, 3, 17, 64, 65, 300, 4095]
IDX_2X3 = [[BIG, [0], [5, 64, 128, 192]], [[1, 2, 3], [64, 128, 4000], BIG]]


def rand_ct(lib, rng, level, B):
    mods = lib.moduli()
    x = np.stack([rng.integers(0, mods[j], (B, 2, lib.N), dtype=np.uint64) for j in range(level + 1)], axis=2)
    return lib.import_ciphertext(x, float(2 ** 40))


def loop(lib, rows, cts):
    outs = []
    for row in rows:
        acc = None
        for t, c in zip(row, cts):
            y = lib.EvaluateLinearTransform(t, c)
            if acc is None:
                acc = y
            else:
                s = lib.AddCiphertextNew(acc, y)
                lib.DeleteCiphertext(acc)
                lib.DeleteCiphertext(y)
                acc = s
        outs.append(lib.RescaleNew(acc))
        lib.DeleteCiphertext(acc)
    return outs


def timed(lib, fn, reps, warm):
    for _ in range(warm):
        for h in fn():
            lib.DeleteCiphertext(h)
    lib.OrionHipSynchronize()
    lib.OrionHipProfileReset()
    lib.OrionHipProfile(1)
    for _ in range(reps):
        for h in fn():
            lib.DeleteCiphertext(h)
    lib.OrionHipSynchronize()
    lib.OrionHipProfile(0)
    prof = lib.profile_read()
    ms = {k: v["ms"] / reps for k, v in prof.items() if v["launches"]}
    n = {k: v["launches"] // reps for k, v in prof.items() if v["launches"]}
    return sum(ms.values()), ms, n


def compare(lib, name, rows, level, args):
    rng = np.random.default_rng(5)
    blk = lib.new_linear_transform_blocks(rows)
    for B in (1, 8):
        cts = [rand_ct(lib, rng, level, B) for _ in rows[0]]
        t_loop, ms_l, n_l = timed(lib, lambda: loop(lib, rows, cts), args.reps, args.warm)
        t_blk, ms_b, n_b = timed(lib, lambda: lib.evaluate_linear_transform_blocks(blk, cts), args.reps, args.warm)
        print(f"{name}  {len(rows)}x{len(rows[0])}  level {level}  B={B}:  loop {t_loop:.3f} ms   blocked {t_blk:.3f} ms"
              f"   loop/blocked {t_loop / t_blk:.2f}")
        for k in sorted(set(ms_l) | set(ms_b)):
            print(f"    {k:14s} loop {n_l.get(k, 0):4d} launches {ms_l.get(k, 0.0):8.3f} ms    "
                  f"blocked {n_b.get(k, 0):4d} launches {ms_b.get(k, 0.0):8.3f} ms")
        for c in cts:
            lib.DeleteCiphertext(c)
    lib.delete_linear_transform_blocks(blk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    args = ap.parse_args()

    st = OrionStream("resnet20_n13", seed=5)
    g = min((g for g in block_groups(st._events) if (g["rows"], g["cols"]) == (4, 4)), key=lambda g: g["start"])
    used = {t for row in g["lts"] for t in row}
    level = {e["ret"]: e["args"][2] for e in st._events
             if e["phase"] == "compile" and e["op"] == "GenerateLinearTransform"}[g["lts"][0][0]]
    st._events = [e for e in st._events if e["phase"] == "compile" and e["op"] == "GenerateLinearTransform" and
                  e["ret"] in used]
    st.keygen()
    st.compile()
    compare(st.lib, "resnet20_n13 conv", [[st.lt_map[t] for t in row] for row in g["lts"]], level, args)
    st.lib.DeleteScheme()

    lib = HipLibrary().new_scheme(13, [55, 40, 40, 40, 40, 40], [60, 60], 40, h=192, seed=6)
    lib.GenerateSecretKey()
    lib.GeneratePublicKey()
    rng = np.random.default_rng(7)
    rows = []
    for irow in IDX_2X3:
        rows.append([])
        for idx in irow:
            d = rng.uniform(-1, 1, (len(idx), lib.slots)).astype(np.float32)
            rows[-1].append(lib.GenerateLinearTransform(idx, list(d.reshape(-1)), 3, 4.0, "none"))
    lib.GenerateConsolidatedRotationKeys(sorted({g for r in rows for t in r for g in lib.GetLinearTransformRotationKeys(t)}))
    compare(lib, "synthetic", rows, 3, args)
    lib.DeleteScheme()


if __name__ == "__main__":
    main()
