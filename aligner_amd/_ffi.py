"""ctypes binding of the C ABI in include/aligner_hip.h (aligner_amd/lib/libaligner_hip.so).

This is the only door between the Python host mirror and the native HIP path.  It fails loudly when the shared
library is missing: there is no Python or CPU implementation of the DP behind it.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ALN_LIB") or os.path.join(_HERE, "lib", "libaligner_hip.so")

# enum aln_semantics
CORE_GLOBAL, CORE_LOCAL, LEGACY_GLOBAL, LEGACY_LOCAL, PWM_LOCAL = 0, 1, 2, 3, 4
# enum aln_status
OK = 0
ERR_UNNECESSARY_ARGUMENT = 1
ERR_EMPTY_SEQUENCE = 2
ERR_CODE_OUT_OF_RANGE = 3
ERR_NO_POSITIVE_CELL = 4
ERR_DEVICE = 5
ERR_OOM = 6
ERR_INVALID_ARGUMENT = 7
ERR_UNSUPPORTED = 8
ERR_MATRIX_SHAPE = 9
ERR_CAPACITY = 10
STATUS_NAMES = {0: "OK", 1: "ERR_UNNECESSARY_ARGUMENT", 2: "ERR_EMPTY_SEQUENCE", 3: "ERR_CODE_OUT_OF_RANGE",
                4: "ERR_NO_POSITIVE_CELL", 5: "ERR_DEVICE", 6: "ERR_OOM", 7: "ERR_INVALID_ARGUMENT",
                8: "ERR_UNSUPPORTED", 9: "ERR_MATRIX_SHAPE", 10: "ERR_CAPACITY"}
# enum aln_outputs
OUT_SCORE, OUT_TRACEBACK, OUT_DIRECTIONS, OUT_H_MATRIX = 1, 2, 4, 8
# aln_seqset_best
SEQSET_BEST_MAX = 64
BEST_SKIP_SELF = 1

# every symbol include/aligner_hip.h declares
EXPORTS = [
    "aln_create", "aln_create_multi", "aln_device_count", "aln_destroy", "aln_last_error", "aln_abi_version", "aln_device_info", "aln_align_pair",
    "aln_align_batch", "aln_plan_chunks", "aln_batch_create", "aln_batch_run", "aln_batch_sync", "aln_batch_fetch",
    "aln_batch_destroy", "aln_batch_cells", "aln_batch_size", "aln_batch_results_device",
    "aln_batch_direction_bytes", "aln_batch_timing", "aln_batch_enable_timing",
    "aln_scan_create", "aln_scan_destroy", "aln_scan_windows", "aln_scan_score", "aln_scan_select", "aln_scan_string_stride",
    "aln_scan_stats", "aln_scan_hits", "aln_scan_held_list", "aln_scan_held_frequencies", "aln_scan_held_strings", "aln_shuffle_scores", "aln_shuffle_targets",
    "aln_pairset_create", "aln_pairset_run", "aln_pairset_frequencies", "aln_pairset_strings", "aln_pairset_stats", "aln_pairset_destroy",
    "aln_transform_matrices",
    "aln_pairset_heuristics", "aln_pairset_reestimate", "aln_pairset_run_stored", "aln_pairset_matrices", "aln_transform_matrices_device",
    "aln_seqset_create", "aln_seqset_destroy", "aln_seqset_pairs", "aln_seqset_score", "aln_seqset_hits", "aln_seqset_held_list",
    "aln_seqset_held_strings", "aln_seqset_stats", "aln_seqset_best", "aln_seqset_held_significance",
    "aln_seqset_held_report", "aln_seqset_held_filter",
    "aln_pairset_create_from_set", "aln_pairset_loop_begin", "aln_pairset_loop_step",
]
# every symbol the companion header include/aligner_hip_cluster.h declares (the same library; the main header's list is pinned)
CLUSTER_EXPORTS = ["aln_cluster_edges", "aln_seqset_held_cluster"]
CLUSTER_COMPONENTS, CLUSTER_GREEDY = 0, 1       # ALN_CLUSTER_COMPONENTS, ALN_CLUSTER_GREEDY
CLUSTER_NONE = 0xFFFFFFFF                       # ALN_CLUSTER_NONE
CLUSTER_MAX = 0xFFFFFFF0                        # nodes, edges
# every symbol the companion header include/aligner_hip_prefilter.h declares (the same library, as above)
PREFILTER_EXPORTS = ["aln_seqset_kmer_index", "aln_seqset_prefilter", "aln_seqset_candidates", "aln_seqset_candidate_scores",
                     "aln_seqset_candidate_hits"]
PREFILTER_MAX_K, PREFILTER_MAX_BITS, PREFILTER_CHUNK_PAIRS = 8, 1 << 18, 1 << 22      # aligner_amd/csrc/aln_prefilter_rules.h
PREFILTER_MAX_CANDIDATES = 0xFFFFFFF0
# every symbol the companion header include/aligner_hip_wordjoin.h declares (the same library, as above)
WORDJOIN_EXPORTS = ["aln_seqset_word_index", "aln_seqset_word_join"]
WORDJOIN_MAX_K, WORDJOIN_MAX_WORDS = 8, 1 << 32             # aligner_amd/csrc/aln_wordjoin_rules.h
WORDJOIN_CHUNK_OCCURRENCES, WORDJOIN_MAX_CHUNK_OCCURRENCES = 1 << 24, 1 << 26
# every symbol the companion header include/aligner_hip_seedjoin.h declares (the same library, as above)
SEEDJOIN_EXPORTS = ["aln_seqset_candidate_diags", "aln_seqset_seed_index", "aln_seqset_seed_join"]
SEEDJOIN_MAX_K, SEEDJOIN_MAX_WORDS, SEEDJOIN_MAX_BAND = 16, 1 << 32, (1 << 31) - 1        # aligner_amd/csrc/aln_seedjoin_rules.h
SEEDJOIN_CHUNK_SEEDS, SEEDJOIN_MAX_CHUNK_SEEDS = 1 << 24, 1 << 26
# every symbol the companion header include/aligner_hip_seedchain.h declares (the same library, as above)
SEEDCHAIN_EXPORTS = ["aln_seqset_candidate_chain_filter", "aln_seqset_candidate_chain_records", "aln_seqset_candidate_chains"]
SEEDCHAIN_MAX_GAP, SEEDCHAIN_MAX_SKEW, SEEDCHAIN_MAX_GAP_SCALE = (1 << 31) - 1, (1 << 31) - 1, 255        # aligner_amd/csrc/aln_seedchain_rules.h
SEEDCHAIN_PAIR_SEEDS, SEEDCHAIN_MAX_PAIR_SEEDS, SEEDCHAIN_CHUNK_ANCHORS, SEEDCHAIN_MAX_CHUNK_ANCHORS = 1 << 16, 1 << 20, 1 << 24, 1 << 26
CHAIN_OVERFLOW = 1
# every symbol the companion header include/aligner_hip_search.h declares (the same library, as above)
SEARCH_EXPORTS = ["aln_seqset_candidate_best"]
# every symbol the companion header include/aligner_hip_profile.h declares (the same library, as above)
PROFILE_EXPORTS = ["aln_seqset_profile_elements", "aln_seqset_held_profiles"]
PROFILE_SKIP_SEED = 1           # ALN_PROFILE_SKIP_SEED
PROFILE_MAX_CODES = 64          # ALN_PROFILE_MAX_CODES
# every symbol the companion header include/aligner_hip_msa.h declares (the same library, as above)
MSA_EXPORTS = ["aln_seqset_held_msa_fill", "aln_seqset_held_msa_plan"]
# every symbol the companion header include/aligner_hip_cigar.h declares (the same library, as above)
CIGAR_EXPORTS = ["aln_seqset_held_cigar_fill", "aln_seqset_held_cigar_plan"]
CIGAR_EXTENDED = 1              # ALN_CIGAR_EXTENDED
CIGAR_CLIPS = 2                 # ALN_CIGAR_CLIPS
# every symbol the companion header include/aligner_hip_strand.h declares (the same library, as above)
STRAND_EXPORTS = ["aln_seqset_create_stranded", "aln_seqset_held_strand_cigar_fill", "aln_seqset_held_strand_cigar_plan",
                  "aln_seqset_strand_records", "aln_seqset_strand_residues"]
PAIRSET_MAX_ENTRIES = 1024      # ALN_PAIRSET_MAX_ENTRIES
TRANSFORM_NO_ROOT = 1           # ALN_TRANSFORM_NO_ROOT
# aln_pairset_loop_step's causes (aligner_amd/csrc/aln_loop_rules.h)
LOOP_CAUSE_DONE, LOOP_CAUSE_FAILED, LOOP_CAUSE_NO_ROOT = 0, 1, 2


class Params(C.Structure):
    _fields_ = [("semantics", C.c_int32), ("heuristics_present", C.c_int32), ("del_", C.c_double),
                ("ext", C.c_double), ("matrix", C.c_void_p), ("rows", C.c_uint32), ("cols", C.c_uint32),
                ("row_stride", C.c_int64), ("outputs", C.c_uint32), ("blank_code", C.c_uint8),
                ("force_f64", C.c_uint8), ("force_serial", C.c_uint8), ("force_generic", C.c_uint8),
                ("max_passes", C.c_uint32)]


class PairResult(C.Structure):
    _fields_ = [("f", C.c_double), ("score", C.c_double), ("end_y", C.c_uint32), ("end_x", C.c_uint32),
                ("start_y", C.c_uint32), ("start_x", C.c_uint32), ("aln_len", C.c_uint32), ("status", C.c_int32),
                ("passes", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(PairResult) == 48

# PairResult.flags / RESULT_DTYPE["flags"] (include/aligner_hip.h): which kernels filled the pair
FLAG_INTEGER = 1        # integer kernels (also a dyadic real-valued scheme, filled scaled by 2^k)
FLAG_SINGLE = 2         # the strip-pipelined single-pair route
FLAG_WORKGROUP = 4      # generic kernels, one workgroup per pair
FLAG_FAST = 8           # the fast integer kernels (i32 keys 4*H + tag, int8 query profile)


class ScanGeometry(C.Structure):
    _fields_ = [("first", C.c_uint64), ("step", C.c_uint64), ("width", C.c_uint64), ("reverse", C.c_uint32),
                ("reserved", C.c_uint32)]



class ShuffleSpec(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("pair_base", C.c_uint64), ("per_pair", C.c_uint32), ("max_trim", C.c_uint32)]


assert C.sizeof(ShuffleSpec) == 24


class SignifRecord(C.Structure):
    """aln_signif_record: what the shuffled copies of one held hit leave behind (aligner_amd/csrc/aln_signif_rules.h)."""
    _fields_ = [("sum", C.c_double), ("sum_sq", C.c_double), ("f_max", C.c_double), ("n_ok", C.c_uint32), ("n_ge", C.c_uint32),
                ("status", C.c_int32), ("first_bad", C.c_uint32), ("reserved", C.c_uint64)]


assert C.sizeof(SignifRecord) == 48
SHUFFLE_MAX_COPIES = 1 << 20      # per pair (aln_shuffle_spec.per_pair)
REPORT_SKIP_SEED = 1              # ALN_REPORT_SKIP_SEED


class HitReport(C.Structure):
    """aln_hit_report: the classed columns of one held hit (aligner_amd/csrc/aln_report_rules.h)."""
    _fields_ = [("columns", C.c_uint32), ("identical", C.c_uint32), ("positive", C.c_uint32), ("mismatch", C.c_uint32),
                ("q_gap", C.c_uint32), ("t_gap", C.c_uint32), ("q_gap_open", C.c_uint32), ("t_gap_open", C.c_uint32),
                ("status", C.c_int32), ("reserved", C.c_uint32)]


class HitFilter(C.Structure):
    """aln_hit_filter: the thresholds of aln_seqset_held_filter."""
    _fields_ = [("min_identity", C.c_double), ("min_q_cover", C.c_double), ("min_t_cover", C.c_double), ("min_columns", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(HitReport) == 40 and C.sizeof(HitFilter) == 32


class ClusterRecord(C.Structure):
    """aln_cluster_record: one cluster of the list (aligner_amd/csrc/aln_cluster_rules.h)."""
    _fields_ = [("label", C.c_uint32), ("size", C.c_uint32), ("longest", C.c_uint32), ("edges", C.c_uint32)]


class ClusterSummary(C.Structure):
    """aln_cluster_summary: the counts of one clustering call."""
    _fields_ = [("nodes", C.c_uint64), ("clusters", C.c_uint64), ("edges", C.c_uint64), ("self_edges", C.c_uint64),
                ("singletons", C.c_uint64), ("rounds", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(ClusterRecord) == 16 and C.sizeof(ClusterSummary) == 48


class ProfileRecord(C.Structure):
    """aln_profile_record: one centre's counters (aligner_amd/csrc/aln_profile_rules.h)."""
    _fields_ = [("center", C.c_uint32), ("hits", C.c_uint32), ("matched", C.c_uint32), ("deleted", C.c_uint32)]


class ProfileSummary(C.Structure):
    """aln_profile_summary: the counts of one profile call."""
    _fields_ = [("held", C.c_uint64), ("contributing", C.c_uint64), ("self_pairs", C.c_uint32), ("between_members", C.c_uint32),
                ("unlisted", C.c_uint32), ("overflow", C.c_uint32), ("elements", C.c_uint64), ("reserved", C.c_uint64)]


assert C.sizeof(ProfileRecord) == 16 and C.sizeof(ProfileSummary) == 48


class MsaRecord(C.Structure):
    """aln_msa_record: one family alignment's shape (aligner_amd/csrc/aln_msa_rules.h)."""
    _fields_ = [("center", C.c_uint32), ("rows", C.c_uint32), ("width", C.c_uint32), ("inserted", C.c_uint32)]


class MsaSummary(C.Structure):
    """aln_msa_summary: the counts and totals of one plan."""
    _fields_ = [("held", C.c_uint64), ("contributing", C.c_uint64), ("self_pairs", C.c_uint32), ("between_members", C.c_uint32),
                ("unlisted", C.c_uint32), ("overflow", C.c_uint32), ("bytes", C.c_uint64), ("total_rows", C.c_uint64)]


assert C.sizeof(MsaRecord) == 16 and C.sizeof(MsaSummary) == 48


class CigarRecord(C.Structure):
    """aln_cigar_record: one listed hit's coordinates and counts (aligner_amd/csrc/aln_cigar_rules.h)."""
    _fields_ = [("n_ops", C.c_uint32), ("q_start", C.c_uint32), ("q_end", C.c_uint32), ("t_start", C.c_uint32), ("t_end", C.c_uint32),
                ("matches", C.c_uint32), ("block", C.c_uint32), ("status", C.c_int32)]


class CigarSummary(C.Structure):
    """aln_cigar_summary: the counts and the total of one plan."""
    _fields_ = [("held", C.c_uint64), ("listed", C.c_uint64), ("total_ops", C.c_uint64), ("failed", C.c_uint32), ("padded", C.c_uint32),
                ("overflow", C.c_uint32), ("reserved", C.c_uint32 * 3)]


assert C.sizeof(CigarRecord) == 32 and C.sizeof(CigarSummary) == 48


class StrandRecord(C.Structure):
    """aln_strand_record: which original records and which strand a listed hit of a stranded set is on (aligner_amd/csrc/aln_strand_rules.h)."""
    _fields_ = [("q_rec", C.c_uint32), ("t_rec", C.c_uint32), ("strand", C.c_uint8), ("q_mirror", C.c_uint8), ("t_mirror", C.c_uint8),
                ("reserved", C.c_uint8), ("reserved2", C.c_uint32)]


assert C.sizeof(StrandRecord) == 16


class PrefilterSpec(C.Structure):
    """aln_prefilter_spec: the index a prefilter call expects and its thresholds (include/aligner_hip_prefilter.h)."""
    _fields_ = [("k", C.c_uint32), ("alphabet", C.c_uint32), ("min_shared", C.c_uint32), ("min_per_1024", C.c_uint32),
                ("chunk_pairs", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


assert C.sizeof(PrefilterSpec) == 32


class WordjoinSpec(C.Structure):
    """aln_wordjoin_spec: the word index a join expects and its thresholds (include/aligner_hip_wordjoin.h)."""
    _fields_ = [("k", C.c_uint32), ("alphabet", C.c_uint32), ("min_shared", C.c_uint32), ("min_per_1024", C.c_uint32),
                ("chunk_occurrences", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


assert C.sizeof(WordjoinSpec) == 32


class SeedjoinSpec(C.Structure):
    """aln_seedjoin_spec: the seed index a join expects, its thresholds and its band (include/aligner_hip_seedjoin.h)."""
    _fields_ = [("k", C.c_uint32), ("alphabet", C.c_uint32), ("min_seeds", C.c_uint32), ("band", C.c_uint32), ("max_occ", C.c_uint32),
                ("chunk_seeds", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class SeedchainSpec(C.Structure):
    """aln_seedchain_spec: the seed index a chaining call expects and the chain's parameters (include/aligner_hip_seedchain.h)."""
    _fields_ = [("k", C.c_uint32), ("alphabet", C.c_uint32), ("max_occ", C.c_uint32), ("max_gap", C.c_uint32), ("max_skew", C.c_uint32),
                ("gap_scale", C.c_uint32), ("max_pair_seeds", C.c_uint32), ("chunk_anchors", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class ChainRecord(C.Structure):
    """aln_chain_record: one candidate's chain."""
    _fields_ = [("score", C.c_int32), ("anchors", C.c_uint32), ("q_start", C.c_uint32), ("q_end", C.c_uint32), ("t_start", C.c_uint32),
                ("t_end", C.c_uint32), ("seeds", C.c_uint32), ("flags", C.c_uint32)]


class SeedchainSummary(C.Structure):
    """aln_seedchain_summary: the counts of one chaining call."""
    _fields_ = [("anchors", C.c_uint64), ("with_anchor", C.c_uint64), ("overflowed", C.c_uint64), ("chunks", C.c_uint64)]


class SeedjoinSummary(C.Structure):
    """aln_seedjoin_summary: the counts of one seed join."""
    _fields_ = [("seeds", C.c_uint64), ("pairs_with_seed", C.c_uint64), ("words_dropped", C.c_uint64), ("chunks", C.c_uint64)]


assert C.sizeof(SeedjoinSpec) == 32 and C.sizeof(SeedjoinSummary) == 32


class SeqsetBlock(C.Structure):
    _fields_ = [("q_first", C.c_uint64), ("q_count", C.c_uint64), ("t_first", C.c_uint64), ("t_count", C.c_uint64),
                ("upper", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(SeqsetBlock) == 40

_lib = None


def load():
    """Loads the native library; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "aligner_amd: native library %s is missing -- run `python -m aligner_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback for the DP path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i, u64p = C.c_void_p, C.c_int, C.c_void_p
    lib.aln_create.restype = vp
    lib.aln_create.argtypes = [i, C.POINTER(C.c_int)]
    lib.aln_create_multi.restype = vp
    lib.aln_create_multi.argtypes = [i, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.aln_device_count.restype = i
    lib.aln_device_count.argtypes = [vp]
    lib.aln_destroy.restype = None
    lib.aln_destroy.argtypes = [vp]
    lib.aln_last_error.restype = C.c_char_p
    lib.aln_last_error.argtypes = []
    lib.aln_abi_version.restype = i
    lib.aln_abi_version.argtypes = []
    lib.aln_device_info.restype = i
    lib.aln_device_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    lib.aln_align_pair.restype = i
    lib.aln_align_pair.argtypes = [vp, C.POINTER(Params), vp, C.c_size_t, vp, C.c_size_t, C.POINTER(PairResult), vp,
                                   vp, vp, vp]
    lib.aln_align_batch.restype = i
    lib.aln_align_batch.argtypes = [vp, C.POINTER(Params), vp, u64p, u64p, u64p, u64p, C.c_size_t, vp, vp, u64p]
    lib.aln_plan_chunks.restype = C.c_size_t
    lib.aln_plan_chunks.argtypes = [C.POINTER(Params), u64p, u64p, C.c_size_t, i, u64p, u64p, C.c_size_t]
    lib.aln_batch_create.restype = vp
    lib.aln_batch_create.argtypes = [vp, C.POINTER(Params), vp, u64p, u64p, u64p, u64p, C.c_size_t,
                                     C.POINTER(C.c_int)]
    lib.aln_batch_run.restype = i
    lib.aln_batch_run.argtypes = [vp, vp]
    lib.aln_batch_sync.restype = i
    lib.aln_batch_sync.argtypes = [vp]
    lib.aln_batch_fetch.restype = i
    lib.aln_batch_fetch.argtypes = [vp, vp, vp, u64p]
    lib.aln_batch_destroy.restype = None
    lib.aln_batch_destroy.argtypes = [vp]
    lib.aln_batch_cells.restype = C.c_uint64
    lib.aln_batch_cells.argtypes = [vp]
    lib.aln_batch_size.restype = C.c_size_t
    lib.aln_batch_size.argtypes = [vp]
    lib.aln_batch_results_device.restype = vp
    lib.aln_batch_results_device.argtypes = [vp]
    lib.aln_batch_direction_bytes.restype = C.c_uint64
    lib.aln_batch_direction_bytes.argtypes = [vp]
    lib.aln_batch_timing.restype = i
    lib.aln_batch_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    lib.aln_batch_enable_timing.restype = None
    lib.aln_batch_enable_timing.argtypes = [vp, i]
    gp = C.POINTER(ScanGeometry)
    lib.aln_scan_create.restype = vp
    lib.aln_scan_create.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int)]
    lib.aln_scan_destroy.restype = None
    lib.aln_scan_destroy.argtypes = [vp]
    lib.aln_scan_windows.restype = C.c_size_t
    lib.aln_scan_windows.argtypes = [vp, gp]
    lib.aln_scan_score.restype = i
    lib.aln_scan_score.argtypes = [vp, C.POINTER(Params), gp, vp]
    lib.aln_scan_select.restype = i
    lib.aln_scan_select.argtypes = [vp, C.POINTER(Params), gp, C.c_double, C.c_double, C.c_double, C.c_size_t,
                                    C.POINTER(C.c_uint64), vp, vp, vp]
    lib.aln_scan_hits.restype = i
    lib.aln_scan_hits.argtypes = [vp, C.POINTER(Params), gp, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_uint64)]
    lib.aln_scan_held_list.restype = i
    lib.aln_scan_held_list.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp]
    lib.aln_scan_held_frequencies.restype = i
    lib.aln_scan_held_frequencies.argtypes = [vp, vp, C.c_uint64, vp]
    lib.aln_scan_held_strings.restype = i
    lib.aln_scan_held_strings.argtypes = [vp, vp, C.c_uint64, vp, vp]
    lib.aln_scan_string_stride.restype = C.c_uint64
    lib.aln_scan_string_stride.argtypes = [vp, C.c_uint32, gp]
    lib.aln_scan_stats.restype = i
    lib.aln_scan_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    sp = C.POINTER(ShuffleSpec)
    lib.aln_shuffle_scores.restype = i
    lib.aln_shuffle_scores.argtypes = [vp, C.POINTER(Params), sp, vp, u64p, u64p, u64p, u64p, C.c_size_t, vp, vp, vp]
    lib.aln_shuffle_targets.restype = i
    lib.aln_shuffle_targets.argtypes = [vp, sp, vp, u64p, u64p, C.c_size_t, vp, u64p]
    lib.aln_pairset_create.restype = vp
    lib.aln_pairset_create.argtypes = [vp, vp, u64p, u64p, u64p, u64p, C.c_size_t, C.POINTER(C.c_int)]
    lib.aln_pairset_run.restype = i
    lib.aln_pairset_run.argtypes = [vp, C.POINTER(Params), vp, vp, C.c_size_t, vp]
    lib.aln_pairset_frequencies.restype = i
    lib.aln_pairset_frequencies.argtypes = [vp, vp, C.c_size_t, vp]
    lib.aln_pairset_strings.restype = i
    lib.aln_pairset_strings.argtypes = [vp, vp, C.c_size_t, vp, vp, u64p]
    lib.aln_pairset_stats.restype = i
    lib.aln_pairset_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.aln_pairset_destroy.restype = None
    lib.aln_pairset_destroy.argtypes = [vp]
    lib.aln_transform_matrices.restype = i
    lib.aln_transform_matrices.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    lib.aln_pairset_heuristics.restype = i
    lib.aln_pairset_heuristics.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    lib.aln_pairset_reestimate.restype = i
    lib.aln_pairset_reestimate.argtypes = [vp, vp, vp, C.c_size_t, vp]
    lib.aln_pairset_run_stored.restype = i
    lib.aln_pairset_run_stored.argtypes = [vp, C.POINTER(Params), vp, C.c_size_t, vp]
    lib.aln_pairset_matrices.restype = i
    lib.aln_pairset_matrices.argtypes = [vp, vp, C.c_size_t, vp]
    lib.aln_transform_matrices_device.restype = i
    lib.aln_transform_matrices_device.argtypes = [vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp]
    bp = C.POINTER(SeqsetBlock)
    lib.aln_seqset_create.restype = vp
    lib.aln_seqset_create.argtypes = [vp, vp, u64p, u64p, C.c_size_t, C.POINTER(C.c_int)]
    lib.aln_seqset_destroy.restype = None
    lib.aln_seqset_destroy.argtypes = [vp]
    lib.aln_seqset_pairs.restype = C.c_uint64
    lib.aln_seqset_pairs.argtypes = [vp, bp]
    lib.aln_seqset_score.restype = i
    lib.aln_seqset_score.argtypes = [vp, C.POINTER(Params), bp, vp, vp]
    lib.aln_seqset_hits.restype = i
    lib.aln_seqset_hits.argtypes = [vp, C.POINTER(Params), bp, C.c_double, C.POINTER(C.c_uint64)]
    lib.aln_seqset_best.restype = i
    lib.aln_seqset_best.argtypes = [vp, C.POINTER(Params), bp, C.c_uint32, C.c_double, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.aln_seqset_held_list.restype = i
    lib.aln_seqset_held_list.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp]
    lib.aln_seqset_held_strings.restype = i
    lib.aln_seqset_held_strings.argtypes = [vp, vp, C.c_uint64, vp, vp, u64p]
    lib.aln_seqset_held_significance.restype = i
    lib.aln_seqset_held_significance.argtypes = [vp, C.POINTER(Params), sp, vp, C.c_uint64, vp, vp, vp]
    lib.aln_seqset_held_report.restype = i
    lib.aln_seqset_held_report.argtypes = [vp, C.POINTER(Params), C.c_uint32, vp, C.c_uint64, vp]
    lib.aln_seqset_held_filter.restype = i
    lib.aln_seqset_held_filter.argtypes = [vp, C.POINTER(Params), C.c_uint32, C.POINTER(HitFilter), vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.aln_seqset_stats.restype = i
    lib.aln_seqset_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.aln_pairset_create_from_set.restype = vp
    lib.aln_pairset_create_from_set.argtypes = [vp, bp, C.c_uint64, C.c_uint64, C.POINTER(C.c_int)]
    lib.aln_pairset_loop_begin.restype = i
    lib.aln_pairset_loop_begin.argtypes = [vp, vp, vp]
    lib.aln_pairset_loop_step.restype = i
    lib.aln_pairset_loop_step.argtypes = [vp, C.POINTER(Params), vp, vp, vp, vp]
    lib.aln_cluster_edges.restype = i
    lib.aln_cluster_edges.argtypes = [vp, C.c_uint32, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(ClusterSummary)]
    lib.aln_seqset_held_cluster.restype = i
    lib.aln_seqset_held_cluster.argtypes = [vp, C.POINTER(Params), C.c_uint32, C.POINTER(HitFilter), C.c_uint32, vp, vp, C.c_uint64,
                                            C.POINTER(ClusterSummary)]
    lib.aln_seqset_kmer_index.restype = i
    lib.aln_seqset_kmer_index.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    lib.aln_seqset_prefilter.restype = i
    lib.aln_seqset_prefilter.argtypes = [vp, C.POINTER(PrefilterSpec), bp, C.POINTER(C.c_uint64)]
    lib.aln_seqset_word_index.restype = i
    lib.aln_seqset_word_index.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    lib.aln_seqset_word_join.restype = i
    lib.aln_seqset_word_join.argtypes = [vp, C.POINTER(WordjoinSpec), bp, C.POINTER(C.c_uint64)]
    lib.aln_seqset_seed_index.restype = i
    lib.aln_seqset_seed_index.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.aln_seqset_seed_join.restype = i
    lib.aln_seqset_seed_join.argtypes = [vp, C.POINTER(SeedjoinSpec), bp, C.POINTER(SeedjoinSummary), C.POINTER(C.c_uint64)]
    lib.aln_seqset_candidate_diags.restype = i
    lib.aln_seqset_candidate_diags.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    lib.aln_seqset_candidate_chains.restype = i
    lib.aln_seqset_candidate_chains.argtypes = [vp, C.POINTER(SeedchainSpec), C.c_uint64, C.c_uint64, vp, C.POINTER(SeedchainSummary)]
    lib.aln_seqset_candidate_chain_filter.restype = i
    lib.aln_seqset_candidate_chain_filter.argtypes = [vp, C.POINTER(SeedchainSpec), C.c_int32, C.c_uint32, C.POINTER(SeedchainSummary), C.POINTER(C.c_uint64)]
    lib.aln_seqset_candidate_chain_records.restype = i
    lib.aln_seqset_candidate_chain_records.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    lib.aln_seqset_candidates.restype = i
    lib.aln_seqset_candidates.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp]
    lib.aln_seqset_candidate_scores.restype = i
    lib.aln_seqset_candidate_scores.argtypes = [vp, C.POINTER(Params), vp, vp]
    lib.aln_seqset_candidate_hits.restype = i
    lib.aln_seqset_candidate_hits.argtypes = [vp, C.POINTER(Params), C.c_double, C.POINTER(C.c_uint64)]
    lib.aln_seqset_candidate_best.restype = i
    lib.aln_seqset_candidate_best.argtypes = [vp, C.POINTER(Params), C.c_uint32, C.c_double, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.aln_seqset_profile_elements.restype = i
    lib.aln_seqset_profile_elements.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.aln_seqset_held_profiles.restype = i
    lib.aln_seqset_held_profiles.argtypes = [vp, C.POINTER(Params), C.c_uint32, C.POINTER(HitFilter), vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp,
                                             C.POINTER(ProfileSummary)]
    lib.aln_seqset_held_msa_plan.restype = i
    lib.aln_seqset_held_msa_plan.argtypes = [vp, C.POINTER(Params), C.c_uint32, C.POINTER(HitFilter), vp, vp, C.c_uint64, vp, C.POINTER(MsaSummary)]
    lib.aln_seqset_held_msa_fill.restype = i
    lib.aln_seqset_held_msa_fill.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64]
    lib.aln_seqset_held_cigar_plan.restype = i
    lib.aln_seqset_held_cigar_plan.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp, C.POINTER(CigarSummary)]
    lib.aln_seqset_held_cigar_fill.restype = i
    lib.aln_seqset_held_cigar_fill.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64]
    lib.aln_seqset_create_stranded.restype = vp
    lib.aln_seqset_create_stranded.argtypes = [vp, vp, u64p, u64p, C.c_size_t, vp, C.POINTER(C.c_int)]
    lib.aln_seqset_strand_records.restype = C.c_uint64
    lib.aln_seqset_strand_records.argtypes = [vp]
    lib.aln_seqset_strand_residues.restype = i
    lib.aln_seqset_strand_residues.argtypes = [vp, C.c_uint64, C.c_uint64, u64p, vp]
    lib.aln_seqset_held_strand_cigar_plan.restype = i
    lib.aln_seqset_held_strand_cigar_plan.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.POINTER(CigarSummary)]
    lib.aln_seqset_held_strand_cigar_fill.restype = i
    lib.aln_seqset_held_strand_cigar_fill.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64]
    _lib = lib
    return lib


def last_error():
    return (load().aln_last_error() or b"").decode("utf-8", "replace")
