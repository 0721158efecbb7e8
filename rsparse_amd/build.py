"""Build librsparse_wrmf_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

One object per source (compiled in parallel, rebuilt only when the source or a shared header changed), then one link.
In-tree output (rsparse_amd/lib/) so the .so travels with the repo snapshot to the GPU box; the objects live in
rsparse_amd/lib/obj/ (git-ignored like the .so).

    python -m rsparse_amd.build [--force] [--out other.so]

--out links the same objects into another file (a second library to load through RSPARSE_HIP_LIB).
"""
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
SRC = [CSRC / n for n in ("wrmf_kernels.hip", "wrmf_cgq.hip", "wrmf_cgp.hip", "wrmf_ne.hip", "wrmf_chol.hip", "wrmf_chol_wave.hip", "wrmf_chol_mf.hip", "wrmf_cg_mf.hip", "wrmf_chol_lr.hip",
                          "wrmf_topk.hip", "wrmf_topk_large.hip", "wrmf_similar.hip", "wrmf_metrics.hip", "wrmf_hits.hip", "wrmf_lists.hip", "wrmf_diversity.hip", "wrmf_mmr.hip", "wrmf_ranks.hip", "wrmf_score.hip", "wrmf_softals.hip", "wrmf_itemknn.hip", "wrmf_ease.hip", "wrmf_slim.hip", "wrmf_bpr.hip", "wrmf_candidates.hip", "wrmf_sample.hip", "wrmf_sample_weighted.hip", "wrmf_split.hip", "wrmf_confidence.hip", "wrmf_events.hip", "wrmf_explain.hip", "wrmf_init.hip", "wrmf_ingest.hip", "wrmf_nnls.hip", "wrmf_bias.hip", "wrmf_lu.hip",
                          "wrmf_f64.hip", "wrmf_wide.hip", "wrmf_wide_cg.hip", "wrmf_ctx_kernels.hip", "wrmf_schedule.cpp", "wrmf_capi.cpp", "wrmf_f64_capi.cpp", "wrmf_capi_host.cpp", "wrmf_ctx.cpp")]
HEADERS = [CSRC / "wrmf_chol_mf.attrs.csv", CSRC / "wrmf_mf.h", CSRC / "wrmf_internal.h", CSRC / "wrmf_capi_common.h", CSRC / "wrmf_schedule.h", CSRC / "wrmf_device.h", CSRC / "wrmf_sample_team.h", CSRC / "wrmf_wave.h", CSRC / "wrmf_csr_rows.h", CSRC / "wrmf_ldlt.h", CSRC / "wrmf_f64.h", CSRC / "wrmf_topk_plan.h", CSRC / "wrmf_ctx_layout.h", PKG.parent / "include" / "rsparse_wrmf_hip.h"]
DEPS = SRC + HEADERS
OUT = PKG / "lib" / "librsparse_wrmf_hip.so"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]


# wrmf_chol_mf.hip names its accumulator registers itself (a0..a159, inline asm) and needs hipcc to stay out of the accumulator
# file: LLVM's function attribute "amdgpu-agpr-alloc"="0" has no source spelling, the ForceFunctionAttrs pass applies it from a
# csv (function,attribute=value).  The listing of that very compilation is then audited (tools/dbg/acc_audit.py: no
# compiler-generated accumulator-file instruction, nothing touches a register an asm load has in flight, two waves per SIMD);
# if the audit fails -- another compiler, a lost flag -- the file is rebuilt with -DMF_SAFE (tiles above hipcc's own share of the
# accumulator file, one wave per SIMD) and audited again; a build that passes neither is an error, never a silent corruption.
EXTRA_FLAGS = {n: ["-mllvm", "-forceattrs-csv-path=" + str(CSRC / "wrmf_chol_mf.attrs.csv"), "-fno-slp-vectorize"] for n in ("wrmf_chol_mf.hip", "wrmf_cg_mf.hip")}
# wrmf_slim.hip states its coordinate descent in separately rounded float64 operations (rsparse_amd/slim.py): no product may be
# contracted into the sum that follows it
EXTRA_FLAGS["wrmf_slim.hip"] = ["-ffp-contract=off"]
# wrmf_bpr.hip likewise: the score, the sigmoid's polynomial, the gradient sums and the Adagrad update of rsparse_amd/bpr.py are
# separately rounded float64 operations
EXTRA_FLAGS["wrmf_bpr.hip"] = ["-ffp-contract=off"]
AUDITED = {"wrmf_chol_mf.hip", "wrmf_cg_mf.hip"}
REG_LIMIT = {"wrmf_cg_mf.hip": 512}   # (one wave per SIMD by design: 320 accumulator registers per row)
# Kernels that fit two waves per SIMD only without a spill (the 24-quad team kernel of wrmf_cgq.hip keeps 192 registers of
# gathered vectors; a spilling form loses 2x): their compilation reports its resource usage and the build fails
# when one of them spills, uses scratch or passes 256 registers -- another compiler may allocate differently.
NO_SPILL = {"wrmf_cgq.hip": ("14als_cgq_kernelILi128ELi24ELi4ELi4E",),
            # four rows per wave: 128 registers of gathered vectors beside four rows' CG state
            "wrmf_cgp.hip": ("14als_cgp_kernelILb0ELb1ELi16ELb1E",),
            # the tile a thread assembles and factors stays in registers from the first chunk to the last pivot
            "wrmf_explain.hip": ("14explain_kernelIfLi128E",),
            # integer-only, about two dozen registers: scratch here would mean the draw loop lost its registers
            "wrmf_sample.hip": ("13sample_kernelILi64E", "13sample_kernelILi256E"),
            # integer-only: two draws, their searches and the table slots per thread
            "wrmf_sample_weighted.hip": ("22sample_weighted_kernelILi64E", "22sample_weighted_kernelILi256E"),
            # integer-only; the leave-out kernels hold four 64-bit keys per lane and nothing else of size
            # integer lookups and one ballot per chunk: scratch here would mean the per-lane cutoff became an indexed array
            "wrmf_hits.hip": ("18hit_metrics_kernelILb0E", "18hit_metrics_kernelILb1E"),
            # integer gathers, two scans and a ballot per chunk, nothing indexed at run time
            "wrmf_lists.hip": ("19list_metrics_kernelILb0E", "19list_metrics_kernelILb1E"),
            # eight doubles of S per lane and kDivAhead gathered rows: scratch would put the running sum in memory
            "wrmf_diversity.hip": ("21list_diversity_kernelI", "21item_inv_norms_kernelI"),
            # kMmrAhead gathered rows and a few doubles per lane, k dependent steps: scratch would sit inside every step
            "wrmf_mmr.hip": ("10mmr_kernelI",),
            # streaming kernels: four entries, their segments and table entries per thread
            "wrmf_confidence.hip": ("conf_moments_kernel", "conf_moments_finish_kernel", "conf_table_kernel", "conf_apply_kernel"),
            # integer keys, ballots and one running double per lane
            "wrmf_events.hip": ("events_pack_kernel", "events_now_kernel", "events_heads_kernel", "events_reduce_kernel",
                                "events_long_chunks_kernel", "events_long_finish_kernel"),
            # one wave per SIMD, the accumulator file named by hand beside ~250 vector registers: a scratch reload is a counted
            # load that drains the LDS-DMA queue (DESIGN.md 3.2 "Round 6"); the limit is the accumulator file plus the kernel's own
            "wrmf_cg_mf.hip": ("rsparse_hip_als_cg_mf_implicit", "rsparse_hip_als_cg_mf_implicit_any"),
            # eight gathered pieces, the row's own factor twice and three coefficient vectors per lane: scratch would sit
            # between the gather and its two uses
            "wrmf_softals.hip": ("softals_span_kernel", "softals_finish_kernel", "softals_empty_rows_kernel"),
            # integer-only: a few indices per lane in the scatter, two keys and their indices per lane in the select's sort;
            # scratch would mean the key lambda or the sort's exchange went to memory (the weighted forms, whose
            # key adds one double product and sum, are held to the same: 3.29)
            # the evaluation consumers (3.30) hold a cell, its lower bound and two run counters per lane
            "wrmf_itemknn.hip": ("knn_scatter_kernel", "knn_mask_kernel", "knn_select_kernel", "knn_gather_kernel", "knn_cand_select_kernel",
                                 "knn_ranks_kernel"),
            # kAhead 16-byte loads in flight and four running doubles per thread: scratch would sit between a load and its add
            # 
            # the cell scorer (3.32): kAhead 4- or 8-byte loads in flight and one running double per lane; the candidate select
            # holds two keys and their items per lane in the sort's exchange
            "wrmf_ease.hip": ("ease_score_kernel", "ease_gram_rows_kernel", "ease_cells_kernel", "ease_cand_select_kernel",
                              "ease_restrict_kernel"),
            # four doubles of a coordinate per lane in the evaluation, four gathered cells of G in flight in the update: scratch
            # would sit inside the column's serial chain
            "wrmf_slim.hip": ("slim_support_kernel", "14slim_cd_kernelILb1E", "14slim_cd_kernelILb0E"),
            # integer-only sampling and bisections; the gradient kernels keep a destination's running chunk sum and total in
            # double registers (two per 16 coordinates and lane): scratch would sit inside the serial walk
            "wrmf_bpr.hip": ("bpr_sample_kernel", "bpr_z_kernel", "bpr_users_kernel", "bpr_item_chunks_kernel", "bpr_items_kernel",
                             "bpr_copy_kernel", "bpr_segments_kernel", "bpr_chunks_kernel"),
            "wrmf_split.hip": ("split_count_wave_kernel", "split_count_team_kernel", "split_write_wave_kernel", "split_write_team_kernel")}
RESOURCE_FLAG = "-Rpass-analysis=kernel-resource-usage"


def resource_violations(remarks, patterns, limit=256):
    """-> [(mangled name, what)] for the kernels of hipcc's kernel-resource-usage remarks whose name contains one of
    `patterns` and that spill, use scratch or need more than `limit` vector registers; every pattern must match a kernel"""
    import re
    rows, cur = [], None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            rows.append(cur)
        elif ":" in t and cur is not None:
            k, v = t.rsplit(":", 1)
            cur[k.strip()] = v.strip()
    bad = []
    for pat in patterns:
        hit = [r for r in rows if pat in r["name"]]
        if not hit:
            bad.append((pat, "no such kernel in the compilation"))
        for r in hit:
            regs = int(r.get("VGPRs", "0")) + int(r.get("AGPRs", "0"))
            for key in ("VGPRs Spill", "ScratchSize [bytes/lane]"):
                if int(r.get(key, "0")):
                    bad.append((r["name"], "%s = %s" % (key, r[key])))
            if regs > limit:
                bad.append((r["name"], "%d vector registers" % regs))
    return bad


def audit_listing(src, extra, obj):
    sys.path.insert(0, str(PKG.parent / "tools" / "dbg"))
    import acc_audit
    lst = obj.with_suffix(".s")

    def listing(flags, floor):
        cmd = ["hipcc", *FLAGS, *flags, "-S", "--cuda-device-only", str(src), "-o", str(lst)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc -S failed on %s:\n%s" % (src.name, r.stderr[-3000:]))
        acc, flight, _ = acc_audit.audit(str(lst), quiet=True, acc_floor=floor)
        return acc, flight, lst.read_text()
    acc, flight, text = listing(extra, 0)
    import re
    # vector registers + the 160 named accumulator registers <= 256: two waves per SIMD.  Demanded of the kernels that run in
    # the normal case; the `_any` instantiations (some confidence below 1: two operand sets) may take a few registers more
    nfree = re.findall(r"\.amdhsa_kernel (\w+)[\s\S]*?\.amdhsa_next_free_vgpr (\d+)", text)
    limit = REG_LIMIT.get(src.name, 256)
    two_waves = bool(nfree) and all(int(v) <= limit for name, v in nfree if "_any" not in name)
    if acc == 0 and flight == 0 and two_waves:
        return
    print("  %s: audit of the two-waves-per-SIMD build failed (accumulator-file %d, in-flight %d, layout ok %s): rebuilding with -DMF_SAFE"
          % (src.name, acc, flight, two_waves), flush=True)
    safe = ["-DMF_SAFE"]
    cmd = ["hipcc", *FLAGS, *safe, "-c", str(src), "-o", str(obj)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s (MF_SAFE):\n%s" % (src.name, r.stderr[-3000:]))
    # (MF_SAFE: hipcc may spill to a0..a95, the tiles are a96..a255: a compiler access at or above a96 breaks rule 1)
    acc, flight, text = listing(safe, 96)
    if acc or flight:
        raise RuntimeError("%s: the MF_SAFE build fails the audit too (accumulator-file %d, in-flight %d)" % (src.name, acc, flight))


def build(force=False, verbose=False, out=None):
    out = Path(out) if out else OUT
    out.parent.mkdir(exist_ok=True)
    objdir = OUT.parent / "obj"
    objdir.mkdir(parents=True, exist_ok=True)
    src = [s for s in SRC if s.exists()]
    hdr_m = max(h.stat().st_mtime for h in HEADERS)
    todo, objs = [], []
    for s in src:
        o = objdir / (s.stem + ".o")
        objs.append(o)
        if force or not o.exists() or o.stat().st_mtime < max(s.stat().st_mtime, hdr_m):
            todo.append((s, o))
    if not todo and out.exists() and all(out.stat().st_mtime >= o.stat().st_mtime for o in objs):
        return out

    def compile_one(so):
        s, o = so
        t0 = time.time()
        extra = EXTRA_FLAGS.get(s.name, [])
        guard = NO_SPILL.get(s.name)
        cmd = ["hipcc", *FLAGS, *extra, *([RESOURCE_FLAG] if guard else []), "-c", str(s), "-o", str(o)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (s.name, r.stderr[-6000:]))
        if guard:
            bad = resource_violations(r.stderr, guard, REG_LIMIT.get(s.name, 256))
            if bad:
                o.unlink()
                raise RuntimeError("%s: kernels that must not spill do:\n%s" % (s.name, "\n".join("  %s: %s" % b for b in bad)))
        if s.name in AUDITED:
            audit_listing(s, extra, o)
        if verbose:
            print("  %-20s %.1f s" % (s.name, time.time() - t0), flush=True)

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(compile_one, todo))
    cmd = ["hipcc", "--offload-arch=gfx950", "-fPIC", "-shared", *map(str, objs), "-ldl", "-lpthread", "-o", str(out)]
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    outp = argv[argv.index("--out") + 1] if "--out" in argv else None
    t0 = time.time()
    print(build(force="--force" in argv, verbose=True, out=outp), "%.1f s" % (time.time() - t0))
