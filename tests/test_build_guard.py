"""rsparse_amd/build.py fails the build when a kernel listed in NO_SPILL (the 24-quad team kernel of wrmf_cgq.hip, which fits two
waves per SIMD only without a spill) spills, uses scratch or passes 256 vector registers.  The check reads hipcc's
kernel-resource-usage remarks of the compilation it guards; here it is fed remarks of that form, without a compiler."""
from rsparse_amd import build as B

NAME = "_ZN11rsparse_hip12_GLOBAL__N_114als_cgq_kernelILi128ELi24ELi4ELi4ELi0ELb1ELi0ELb0ELb1EEEvNS_7AlsArgsEPKiiim"
OTHER = "_ZN11rsparse_hip12_GLOBAL__N_114als_cgq_kernelILi128ELi16ELi8ELi8ELi0ELb1ELi0ELb0ELb1EEEvNS_7AlsArgsEPKiiim"


def _remarks(name, vgprs, spill, scratch, agprs=0):
    tag = " [-Rpass-analysis=kernel-resource-usage]"
    rows = ["Function Name: " + name, "    SGPRs: 100", "    VGPRs: %d" % vgprs, "    AGPRs: %d" % agprs,
            "    ScratchSize [bytes/lane]: %d" % scratch, "    Dynamic Stack: False", "    Occupancy [waves/SIMD]: 2",
            "    SGPRs Spill: 0", "    VGPRs Spill: %d" % spill, "    LDS Size [bytes/block]: 0"]
    return "\n".join("wrmf_cgq.hip:126:0: remark: " + r + tag for r in rows) + "\n"


def test_the_guard_names_the_wide_team_kernel():
    assert all(p in NAME for p in B.NO_SPILL["wrmf_cgq.hip"])
    assert not any(p in OTHER for p in B.NO_SPILL["wrmf_cgq.hip"])


def test_clean_kernel_passes_and_other_kernels_may_spill():
    text = _remarks(NAME, 256, 0, 0) + _remarks(OTHER, 256, 5, 16)
    assert B.resource_violations(text, B.NO_SPILL["wrmf_cgq.hip"]) == []


def test_spill_scratch_and_register_count_are_reported():
    pats = B.NO_SPILL["wrmf_cgq.hip"]
    bad = B.resource_violations(_remarks(NAME, 256, 6, 28), pats)
    assert [b[0] for b in bad] == [NAME, NAME] and "VGPRs Spill = 6" in bad[0][1] and "ScratchSize" in bad[1][1]
    assert B.resource_violations(_remarks(NAME, 250, 0, 0, agprs=8), pats) == [(NAME, "258 vector registers")]


def test_a_guarded_kernel_that_is_not_compiled_is_reported():
    bad = B.resource_violations(_remarks(OTHER, 200, 0, 0), B.NO_SPILL["wrmf_cgq.hip"])
    assert len(bad) == 1 and "no such kernel" in bad[0][1]
