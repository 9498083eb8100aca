"""Store the reference's own leaf routines (lib_transforms.cpp: Haar, Hadamard, bior1.5; mt19937ar.c: genrand_res53),
compiled unmodified into oracle/_ref/libref_leaf.so by `make -C oracle ref`, on fixed inputs as
tests/golden/ref_leaf_vectors.npz: tests/test_oracle_leaf.py pins the oracle's routines to these outputs bit for bit.
Run where the reference tree is present (the only place oracle/_ref can be built)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as O  # noqa: E402

R = O.ref_lib()
if R is None:
    raise SystemExit("oracle/_ref/libref_leaf.so is not built (make -C oracle ref needs the reference tree)")
rng = np.random.default_rng(7)
out = {}
for n in (1, 2, 4, 8, 16, 32):
    vs = (rng.normal(size=(20, n)) * 100).astype(np.float32)
    out[f"haar_in_{n}"] = vs
    for key, fn in (("haar_fwd", R.ref_haar_forward), ("haar_inv", R.ref_haar_inverse), ("hadamard", R.ref_hadamard)):
        res = vs.copy()
        for row in res:
            fn(row, n)
        out[f"{key}_{n}"] = res
for n in (2, 4, 8, 16):
    imgs = (rng.normal(size=(5, n + 3, n + 5)) * 60 + 128).astype(np.float32)
    fwd, inv = np.zeros((5, n * n), np.float32), np.zeros((5, n * n), np.float32)
    for i, img in enumerate(imgs):
        R.ref_bior_forward(img.reshape(-1), img.shape[1], img.size, fwd[i], n)
        inv[i] = fwd[i]
        R.ref_bior_inverse(inv[i], n)
    out[f"bior_in_{n}"], out[f"bior_fwd_{n}"], out[f"bior_inv_{n}"] = imgs, fwd, inv
seeds = np.array([1, 5489, 123456789], np.uint64)
res53 = np.zeros((len(seeds), 2000), np.float64)
for i, s in enumerate(seeds):
    R.ref_mt_seed(int(s))
    res53[i] = [R.ref_mt_res53() for _ in range(res53.shape[1])]
out["mt_seeds"], out["mt_res53"] = seeds, res53
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ref_leaf_vectors.npz")
np.savez(path, **out)
print("wrote", os.path.normpath(path), sum(v.nbytes for v in out.values()), "bytes")
