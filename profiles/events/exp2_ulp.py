"""The error of the device's double exp2 (read off the kernel's own decay weights) on the arguments of tests/test_events.py::test_decayed_sum_within_the_derived_bound,
in ulps, against np.exp2 in np.longdouble (64-bit significand): the source of EXP2_ULP in that test.

    python profiles/events/exp2_ulp.py
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    import test_events as T
    u, i, v, t, _ = T._log()
    out = {"longdouble_mantissa_bits": int(np.finfo(np.longdouble).nmant)}
    worst = 0.0
    tu = np.unique(t)
    for now in (float(t.max()), 7.25):
        arg = (tu - now) / 1000.0
        dev = T._weights(tu, 1000.0, now)      # the kernel's own exp2: a cell of one event without a value holds its weight
        torch_dev = torch.exp2(torch.from_numpy(arg).cuda()).cpu().numpy()
        host = np.exp2(arg)
        exact = np.exp2(arg.astype(np.longdouble))
        ulp = np.spacing(np.abs(exact).astype(np.float64)).astype(np.longdouble)
        e_dev = float(np.max(np.abs(dev.astype(np.longdouble) - exact) / ulp))
        e_host = float(np.max(np.abs(host.astype(np.longdouble) - exact) / ulp))
        out["now=%g" % now] = {"arguments": int(arg.size), "device_ulp": e_dev, "numpy_ulp": e_host,
                               "device_equals_numpy": int((dev == host).sum()),
                               "device_equals_torch_exp2": int((dev == torch_dev).sum())}
        worst = max(worst, e_dev)
    out["device_ulp_max"] = worst
    out["EXP2_ULP"] = int(np.ceil(worst))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
