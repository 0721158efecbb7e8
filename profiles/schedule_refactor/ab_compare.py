import sys
import numpy as np
a1, a2, b = (np.load(f) for f in sys.argv[1:4])
ok = True
for key in sorted(k[:-2] for k in a1.files if k.endswith("_Y")):
    def diff(u, v):
        return float(np.abs(u[key + "_Y"].astype(np.float64) - v[key + "_Y"]).max(axis=0).max()), u[key + "_Y"].tobytes() == v[key + "_Y"].tobytes() and u[key + "_loss"].tobytes() == v[key + "_loss"].tobytes()
    dpp, same_pp = diff(a1, a2)
    dnp, same_np = diff(b, a1)
    verdict = "bitwise" if same_np else ("within parent-vs-parent" if (not same_pp and dnp <= dpp) else "DIFFERS")
    ok &= verdict != "DIFFERS"
    print("%-14s parent-vs-parent: %s (max |dY| %.3g)   new-vs-parent: %s (max |dY| %.3g)   loss parent %r new %r   -> %s"
          % (key, "bitwise" if same_pp else "differs", dpp, "bitwise" if same_np else "differs", dnp,
             float(a1[key + "_loss"]), float(b[key + "_loss"]), verdict))
sys.exit(0 if ok else 1)
