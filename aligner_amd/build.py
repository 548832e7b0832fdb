"""Builds aligner_amd/lib/libaligner_hip.so (HIP kernels + C ABI) for gfx950 with hipcc.

hipcc cross-compiles without a GPU, so this runs in the dev container; the built .so travels to the GPU box
with the repo snapshot.  `python -m aligner_amd.build [--force] [--remarks]`.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libaligner_hip.so")
SOURCES = ["aln_kernels.hip", "aln_traceback.hip", "aln_host.hip", "aln_scan.hip", "aln_shuffle.hip", "aln_signif.hip", "aln_pairset.hip", "aln_seqset.hip", "aln_loop.hip", "aln_best.hip", "aln_report.hip", "aln_cluster.hip", "aln_prefilter.hip", "aln_search.hip", "aln_profile.hip", "aln_msa.hip", "aln_cigar.hip", "aln_wordjoin.hip", "aln_strand.hip", "aln_seedjoin.hip", "aln_seedchain.hip"]
# aln_kernels.hip (the fills) is compiled as several translation units side by side (-DALN_TU=<mask of its ALN_PART_* families>): the
# fast core-local batch kernel alone is half of the compile time.  fast_rest_solo also holds the two-pairs-per-wave kernel
# (ALN_PART_DUO, 128).  Every other source, aln_traceback.hip included, is one unit.
KERNEL_UNITS = [("generic", 1), ("fast_cl", 2), ("fast_rest", 4), ("single", 8), ("fast_cl_solo", 32), ("fast_rest_solo", 64 | 128)]
HEADERS = ["aln_arena_rules.h", "aln_best_rules.h", "aln_cigar_rules.h", "aln_cluster_rules.h", "aln_device.h", "aln_fast.h", "aln_launch.h", "aln_layout_rules.h", "aln_loop_rules.h", "aln_msa_rules.h", "aln_plan_rules.h", "aln_prefilter_rules.h", "aln_profile_rules.h", "aln_report_rules.h", "aln_scheme_rules.h", "aln_search_rules.h", "aln_select.h", "aln_seqset_rules.h", "aln_shuffle_rules.h", "aln_signif_rules.h", "aln_strand_rules.h", "aln_transform_rules.h", "aln_wordjoin_rules.h", "aln_seedjoin_rules.h", "aln_seedchain_rules.h", "aln_postings.h", "aln_single_unit.inc", os.path.join("..", "..", "include", "aligner_hip.h"),
           os.path.join("..", "..", "include", "aligner_hip_cluster.h"), os.path.join("..", "..", "include", "aligner_hip_prefilter.h"),
           os.path.join("..", "..", "include", "aligner_hip_search.h"), os.path.join("..", "..", "include", "aligner_hip_profile.h"),
           os.path.join("..", "..", "include", "aligner_hip_msa.h"), os.path.join("..", "..", "include", "aligner_hip_cigar.h"),
           os.path.join("..", "..", "include", "aligner_hip_wordjoin.h"), os.path.join("..", "..", "include", "aligner_hip_strand.h"),
           os.path.join("..", "..", "include", "aligner_hip_seedjoin.h"), os.path.join("..", "..", "include", "aligner_hip_seedchain.h")]
# host-only helper of the synthetic workloads (splitmix64 residues; aligner_amd/workloads.py only LOADS it)
SYNTH_LIB = os.path.join(LIBDIR, "libaln_synth.so")
SYNTH_SRC = os.path.join(CSRC, "aln_synth.c")
# -ffp-contract=off: the f64 kernels must be the reference's add/sub/max/compare, never an fma
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-Wall", "-Wno-unused-function"]


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build_synth(force=False):
    if force or not os.path.exists(SYNTH_LIB) or os.path.getmtime(SYNTH_SRC) > os.path.getmtime(SYNTH_LIB):
        os.makedirs(LIBDIR, exist_ok=True)
        tmp = SYNTH_LIB + ".tmp%d" % os.getpid()
        subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared", "-o", tmp, SYNTH_SRC])
        os.replace(tmp, SYNTH_LIB)
    return SYNTH_LIB


# tests/abi_harness.c: include/aligner_hip.h compiled as C99 and linked against the library (the check that the header itself is a
# usable C interface; run on the GPU box by tests/test_gpu_parity.py)
HARNESS_SRC = os.path.join(HERE, "..", "tests", "abi_harness.c")
HARNESS = os.path.join(HERE, "..", "tests", "bin", "abi_harness")


# tests/abi_families.c: the same for every other exported family (tests/test_abi_layout_cpu.py, tests/test_abi_families_gpu.py)
FAMILIES_SRC = os.path.join(HERE, "..", "tests", "abi_families.c")
FAMILIES = os.path.join(HERE, "..", "tests", "bin", "abi_families")
# tests/abi_cluster.c: the same for the companion header include/aligner_hip_cluster.h (tests/test_cluster_rules_cpu.py,
# tests/test_cluster_gpu.py)
CLUSTER_SRC = os.path.join(HERE, "..", "tests", "abi_cluster.c")
CLUSTER = os.path.join(HERE, "..", "tests", "bin", "abi_cluster")
# tests/abi_prefilter.c: the same for the companion header include/aligner_hip_prefilter.h (tests/test_prefilter_rules_cpu.py,
# tests/test_prefilter_gpu.py)
PREFILTER_SRC = os.path.join(HERE, "..", "tests", "abi_prefilter.c")
PREFILTER = os.path.join(HERE, "..", "tests", "bin", "abi_prefilter")
# tests/abi_search.c: the same for the companion header include/aligner_hip_search.h (tests/test_search_rules_cpu.py,
# tests/test_search_gpu.py)
SEARCH_SRC = os.path.join(HERE, "..", "tests", "abi_search.c")
SEARCH = os.path.join(HERE, "..", "tests", "bin", "abi_search")
# tests/abi_profile.c: the same for the companion header include/aligner_hip_profile.h (tests/test_profile_rules_cpu.py,
# tests/test_profile_gpu.py)
PROFILE_SRC = os.path.join(HERE, "..", "tests", "abi_profile.c")
PROFILE = os.path.join(HERE, "..", "tests", "bin", "abi_profile")
# tests/abi_msa.c: the same for the companion header include/aligner_hip_msa.h (tests/test_msa_rules_cpu.py, tests/test_msa_gpu.py)
MSA_SRC = os.path.join(HERE, "..", "tests", "abi_msa.c")
MSA = os.path.join(HERE, "..", "tests", "bin", "abi_msa")
# tests/abi_cigar.c: the same for the companion header include/aligner_hip_cigar.h (tests/test_cigar_rules_cpu.py, tests/test_cigar_gpu.py)
CIGAR_SRC = os.path.join(HERE, "..", "tests", "abi_cigar.c")
CIGAR = os.path.join(HERE, "..", "tests", "bin", "abi_cigar")
# tests/abi_wordjoin.c: the same for the companion header include/aligner_hip_wordjoin.h (tests/test_wordjoin_rules_cpu.py,
# tests/test_wordjoin_gpu.py)
WORDJOIN_SRC = os.path.join(HERE, "..", "tests", "abi_wordjoin.c")
WORDJOIN = os.path.join(HERE, "..", "tests", "bin", "abi_wordjoin")
# tests/abi_strand.c: the same for the companion header include/aligner_hip_strand.h (tests/test_strand_rules_cpu.py,
# tests/test_strand_gpu.py)
STRAND_SRC = os.path.join(HERE, "..", "tests", "abi_strand.c")
STRAND = os.path.join(HERE, "..", "tests", "bin", "abi_strand")
# tests/abi_seedjoin.c: the same for the companion header include/aligner_hip_seedjoin.h (tests/test_seedjoin_rules_cpu.py,
# tests/test_seedjoin_gpu.py)
SEEDJOIN_SRC = os.path.join(HERE, "..", "tests", "abi_seedjoin.c")
SEEDJOIN = os.path.join(HERE, "..", "tests", "bin", "abi_seedjoin")
# tests/abi_seedchain.c: the same for the companion header include/aligner_hip_seedchain.h (tests/test_seedchain_rules_cpu.py,
# tests/test_seedchain_gpu.py)
SEEDCHAIN_SRC = os.path.join(HERE, "..", "tests", "abi_seedchain.c")
SEEDCHAIN = os.path.join(HERE, "..", "tests", "bin", "abi_seedchain")


def build_harness(force=False):
    return _build_c_program(HARNESS_SRC, HARNESS, force)


def build_families_harness(force=False):
    return _build_c_program(FAMILIES_SRC, FAMILIES, force)


def build_cluster_harness(force=False):
    return _build_c_program(CLUSTER_SRC, CLUSTER, force)


def build_prefilter_harness(force=False):
    return _build_c_program(PREFILTER_SRC, PREFILTER, force)


def build_search_harness(force=False):
    return _build_c_program(SEARCH_SRC, SEARCH, force)


def build_profile_harness(force=False):
    return _build_c_program(PROFILE_SRC, PROFILE, force)


def build_msa_harness(force=False):
    return _build_c_program(MSA_SRC, MSA, force)


def build_cigar_harness(force=False):
    return _build_c_program(CIGAR_SRC, CIGAR, force)


def build_wordjoin_harness(force=False):
    return _build_c_program(WORDJOIN_SRC, WORDJOIN, force)


def build_strand_harness(force=False):
    return _build_c_program(STRAND_SRC, STRAND, force)


def build_seedjoin_harness(force=False):
    return _build_c_program(SEEDJOIN_SRC, SEEDJOIN, force)


def build_seedchain_harness(force=False):
    return _build_c_program(SEEDCHAIN_SRC, SEEDCHAIN, force)


def _build_c_program(src, out, force=False):
    src, out = os.path.abspath(src), os.path.abspath(out)
    hdrs = [os.path.join(HERE, "..", "include", h) for h in ("aligner_hip.h", "aligner_hip_cluster.h", "aligner_hip_prefilter.h", "aligner_hip_search.h", "aligner_hip_profile.h", "aligner_hip_msa.h", "aligner_hip_cigar.h", "aligner_hip_wordjoin.h", "aligner_hip_strand.h", "aligner_hip_seedjoin.h", "aligner_hip_seedchain.h")]
    if force or not os.path.exists(out) or max([os.path.getmtime(f) for f in [src, LIB] + hdrs]) > os.path.getmtime(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = out + ".tmp%d" % os.getpid()
        subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(HERE, "..", "include"), src, "-o", tmp,
                               "-L", LIBDIR, "-laligner_hip", "-Wl,-rpath,$ORIGIN/../../aligner_amd/lib", "-Wl,-rpath-link,/opt/rocm/lib"])
        os.replace(tmp, out)
    return out


def build(force=False, remarks=False):
    lib = _build_lib(force, remarks)
    build_harness(force)
    build_families_harness(force)
    build_cluster_harness(force)
    build_prefilter_harness(force)
    build_search_harness(force)
    build_profile_harness(force)
    build_msa_harness(force)
    build_cigar_harness(force)
    build_wordjoin_harness(force)
    build_strand_harness(force)
    build_seedjoin_harness(force)
    build_seedchain_harness(force)
    return lib


def _build_lib(force=False, remarks=False):
    build_synth(force)
    if not force and not needs_build():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "hipcc")
    # ALN_CXXFLAGS: extra flags for an instrumented build (-DALN_STAMPS: per-pair time stamps for tools/tail_timeline.py)
    base = [hipcc] + [f for f in FLAGS if f != "-shared"] + os.environ.get("ALN_CXXFLAGS", "").split() + \
        (["-Rpass-analysis=kernel-resource-usage"] if remarks else [])
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    jobs = [(base + ["-DALN_TU=%d" % mask, "-c", os.path.join(CSRC, "aln_kernels.hip"), "-o", os.path.join(objdir, "aln_kernels_%s.o" % name)])
            for name, mask in KERNEL_UNITS]
    jobs += [base + ["-c", os.path.join(CSRC, src), "-o", os.path.join(objdir, src.replace(".hip", ".o"))] for src in SOURCES if src != "aln_kernels.hip"]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as pool:
        for rc, cmd in zip(pool.map(subprocess.call, jobs), jobs):
            if rc != 0:
                raise subprocess.CalledProcessError(rc, cmd)
    tmp = LIB + ".tmp%d" % os.getpid()
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + [j[-1] for j in jobs] + ["-o", tmp])
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, remarks="--remarks" in sys.argv))
