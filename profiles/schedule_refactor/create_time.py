"""Host clock around rsparse_hip_csc_create_device on the bench matrix, both orientations (library: RSPARSE_HIP_LIB)."""
import ctypes, json, sys, time
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from rsparse_amd import _lib, synth  # noqa: E402
lib = _lib.load()
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
data = synth.make_dataset(10_000_000, 1_000_000, seed=20250222, mean_deg=50.0, device=dev, feedback="implicit")
res = {}
for name, n_rows, n_cols in (("c_ui", data["n_users"], data["n_items"]), ("c_iu", data["n_items"], data["n_users"])):
    p, i, x = data[name]
    ts = []
    for rep in range(4):
        h = ctypes.c_void_p()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(lib.rsparse_hip_csc_create_device(int(n_rows), int(n_cols), p.data_ptr(), i.data_ptr(), x.data_ptr(), ctypes.byref(h)))
        ts.append((time.perf_counter() - t0) * 1e3)
        info = (ctypes.c_int64 * 40)()
        lib.rsparse_hip_csc_info(h, info)
        lib.rsparse_hip_csc_destroy(h)
    res[name + "_ms"] = [round(t, 2) for t in ts]
    res[name + "_info"] = list(info)[:22]
print(json.dumps(res), flush=True)
