"""Seeded half-iterations through the library named by RSPARSE_HIP_LIB; writes Y and loss of every configuration to argv[1]."""
import sys
from pathlib import Path
import numpy as np
sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from rsparse_amd import als  # noqa: E402

rng = np.random.default_rng(11)
n_fix, n_solve = 40000, 700
lens = np.concatenate([[30000, 20000, 16384, 16385, 9000, 5000, 2048, 2047, 1000, 600, 513, 8000, 3000, 12000],
                       rng.integers(0, 513, n_solve - 14)])
lens = lens[rng.permutation(n_solve)]
assert (lens > 16384).sum() >= 1 and ((lens > 512) & (lens <= 16384)).sum() >= 5
p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
i = np.concatenate([np.sort(rng.choice(n_fix, int(l), replace=False)) for l in lens]).astype(np.int32)
x_imp = (1.0 + rng.exponential(2.0, i.size)).astype(np.float32).astype(np.float64)
x_exp = rng.integers(1, 6, i.size).astype(np.float64)
out = {}
for name, k, solver, kind, gb in (("cg128", 128, 1, "imp", 0.0), ("cg64", 64, 1, "imp", 0.0), ("cg64_gbias", 64, 1, "imp", 0.05),
                                  ("chol128", 128, 0, "imp", 0.0), ("chol64", 64, 0, "imp", 0.0), ("cg64_explicit", 64, 1, "exp", 0.0)):
    r = np.random.default_rng(k + solver)
    X = np.asfortranarray((r.standard_normal((k, n_fix)) * 0.05).astype(np.float32))
    Y = np.asfortranarray((r.standard_normal((k, n_solve)) * 0.05).astype(np.float32))
    if kind == "imp":
        loss = als.als_implicit((n_fix, n_solve, p, i, x_imp), X, Y, 0.1, 1, solver, 3, "float", False, False, global_bias=gb)
    else:
        loss = als.als_explicit((n_fix, n_solve, p, i, x_exp), X, Y, None, 0.1, 1, solver, 3, False, "float", False, False)
    assert np.isfinite(Y).all()
    out[name + "_Y"] = Y
    out[name + "_loss"] = np.float64(loss)
    print(name, repr(loss), flush=True)
np.savez(sys.argv[1], **out)
