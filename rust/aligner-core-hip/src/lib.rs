//! MI355X-backed aligners behind the reference's own trait: `HipGlobalAligner`, `HipLocalAligner` (both
//! `AlignerTrait<T, Alignment<T>>`, replacing `simple::{SimpleGlobalAligner, SimpleLocalAligner}`, simple/mod.rs:19-265) and
//! `HipPWMAligner` (`AlignerTrait<T, PWMAlignment<T>>`, replacing `pwm::PWMAligner`, pwm/mod.rs:9-126), plus the batch call
//! that replaces the ten-thread loop of `calculate_p_value` (statistics/mod.rs:255-286).
//! Goes into the reference as `aligner-core/src/hip/mod.rs`.  NOT compiled in the build image (no Rust toolchain there): the C ABI
//! it binds is exercised by tests/abi_harness.c and by the Python binding instead.
use crate::alignment::{Alignment, PWMAlignment};
use crate::alignment_result::AlignmentResult;
use crate::enums::Direction;
use crate::{AlignerTrait, BioData, Error, Heuristics, Result};
use ndarray::Array2;
use std::marker::PhantomData;
use std::os::raw::{c_char, c_int};

// ---------------------------------------------------------------- include/aligner_hip.h
#[repr(C)]
pub struct AlnParams {
    pub semantics: i32,
    pub heuristics_present: i32,
    pub del: f64,
    pub ext: f64,
    pub matrix: *const f64,
    pub rows: u32,
    pub cols: u32,
    pub row_stride: i64,
    pub outputs: u32,
    pub blank_code: u8,
    pub force_f64: u8,
    pub force_serial: u8,
    pub force_generic: u8,
    pub max_passes: u32,
} // 64 bytes
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct AlnPairResult {
    pub f: f64,
    pub score: f64,
    pub end_y: u32,
    pub end_x: u32,
    pub start_y: u32,
    pub start_x: u32,
    pub aln_len: u32,
    pub status: i32,
    pub passes: u32,
    pub flags: u32,
} // 48 bytes
#[repr(C)]
pub struct AlnCtx {
    _p: [u8; 0],
}

extern "C" {
    fn aln_create(device_id: c_int, status: *mut c_int) -> *mut AlnCtx;
    fn aln_create_multi(n_devices: c_int, device_ids: *const c_int, status: *mut c_int) -> *mut AlnCtx;
    fn aln_last_error() -> *const c_char;
    fn aln_align_pair(ctx: *mut AlnCtx, p: *const AlnParams, q: *const u8, n: usize, t: *const u8, m: usize, out: *mut AlnPairResult,
                      q_aln: *mut u8, t_aln: *mut u8, directions: *mut u8, h_matrix: *mut f64) -> c_int;
    fn aln_align_batch(ctx: *mut AlnCtx, p: *const AlnParams, seqs: *const u8, q_off: *const u64, q_len: *const u64, t_off: *const u64,
                       t_len: *const u64, n_pairs: usize, results: *mut AlnPairResult, tb_buf: *mut u8, tb_off: *const u64) -> c_int;
}

/// The window scan of `latent-repeat-search` (include/aligner_hip.h, "window scan"): a chromosome resident on the GPU, passes described
/// by a geometry.  `aln_scan_hits` is the held form of `aln_scan_select`: every hit's summary and strings stay on the device, the count
/// alone comes back (no capacity, no second fill); `aln_scan_held_list` gives window number and f per hit, `aln_scan_held_frequencies`
/// the sum of the listed hits' `get_frequency_matrix()` (counted in unsigned integers on the device: exact, any order), and
/// `aln_scan_held_strings` the summaries and strings of the listed hits only -- what `calculate_cycle` + `filter` + the PWM update of
/// engine/calc.rs:187-216 need.  Held state lasts until the next score / select / hits on the scan.
pub mod scan {
    use super::{AlnCtx, AlnPairResult, AlnParams};
    use std::os::raw::c_int;

    #[repr(C)]
    pub struct AlnScan { _private: [u8; 0] }

    #[repr(C)]
    #[derive(Clone, Copy)]
    pub struct AlnScanGeometry { pub first: u64, pub step: u64, pub width: u64, pub reverse: u32, pub reserved: u32 }

    extern "C" {
        pub fn aln_scan_create(ctx: *mut AlnCtx, seq: *const u8, len: usize, status: *mut c_int) -> *mut AlnScan;
        pub fn aln_scan_destroy(scan: *mut AlnScan);
        pub fn aln_scan_windows(scan: *const AlnScan, g: *const AlnScanGeometry) -> usize;
        pub fn aln_scan_score(scan: *mut AlnScan, p: *const AlnParams, g: *const AlnScanGeometry, f: *mut f64) -> c_int;
        pub fn aln_scan_select(scan: *mut AlnScan, p: *const AlnParams, g: *const AlnScanGeometry, mean: f64, sd: f64, z_min: f64, cap: usize,
                               count: *mut u64, indices: *mut u32, results: *mut AlnPairResult, tb_buf: *mut u8) -> c_int;
        pub fn aln_scan_hits(scan: *mut AlnScan, p: *const AlnParams, g: *const AlnScanGeometry, mean: f64, sd: f64, z_min: f64,
                             count: *mut u64) -> c_int;
        pub fn aln_scan_held_list(scan: *mut AlnScan, first: u64, n: u64, indices: *mut u32, f: *mut f64) -> c_int;
        /// counts: 4 * cols doubles, counts[c * cols + (col - 1)]
        pub fn aln_scan_held_frequencies(scan: *mut AlnScan, keep: *const u32, n_keep: u64, counts: *mut f64) -> c_int;
        pub fn aln_scan_held_strings(scan: *mut AlnScan, keep: *const u32, n_keep: u64, results: *mut AlnPairResult, tb_buf: *mut u8) -> c_int;
        pub fn aln_scan_string_stride(scan: *const AlnScan, cols: u32, g: *const AlnScanGeometry) -> u64;
        pub fn aln_scan_stats(scan: *const AlnScan, ms: *mut f64, bytes: *mut u64) -> c_int;
    }
}

pub const CORE_GLOBAL: i32 = 0;
pub const CORE_LOCAL: i32 = 1;
pub const PWM_LOCAL: i32 = 4;
pub const OUT_SCORE: u32 = 1;
pub const OUT_TRACEBACK: u32 = 2;
pub const OUT_DIRECTIONS: u32 = 4;
pub const OUT_H: u32 = 8;

/// `AlignmentResult.{alignment_matrix, direction_matrix}` are filled only on request: nothing in the reference reads them after
/// construction, and they cost 9 bytes per cell over PCIe.  `false` (the default) leaves both 0 x 0 and runs the fast
/// kernels: 0.31 ms for a 1k x 1k pair against 1.2 ms with both matrices.
pub static WANT_MATRICES: std::sync::atomic::AtomicBool = std::sync::atomic::AtomicBool::new(false);

/// One context per process.  `ALIGNER_HIP_DEVICES=all` (or a multi-GPU host process): every visible GPU behind one context --
/// single calls go to the GPUs in turn, a batch call is sharded over them (`aln_create_multi(0, NULL)`); otherwise the GPU named by
/// `LOCAL_RANK` (one process per GPU, as `torch.distributed.run` / `mpirun` launch them), default 0.
pub fn ctx() -> *mut AlnCtx {
    use std::sync::OnceLock;
    static CTX: OnceLock<usize> = OnceLock::new();
    *CTX.get_or_init(|| {
        let mut st = 0;
        let all = std::env::var("ALIGNER_HIP_DEVICES").map(|v| v == "all").unwrap_or(false);
        let c = if all {
            unsafe { aln_create_multi(0, std::ptr::null(), &mut st) }
        } else {
            let dev = std::env::var("LOCAL_RANK").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
            unsafe { aln_create(dev, &mut st) }
        };
        assert!(!c.is_null(), "aln_create failed ({st}): no MI355X / HIP runtime -- there is no CPU fallback");
        c as usize
    }) as *mut AlnCtx
}

fn params(semantics: i32, del: f64, ext: f64, mat: &Array2<f64>, heuristics: bool, outputs: u32, blank: u8) -> AlnParams {
    AlnParams {
        semantics, heuristics_present: heuristics as i32, del, ext,
        matrix: mat.as_ptr(), rows: mat.nrows() as u32, cols: mat.ncols() as u32, row_stride: mat.ncols() as i64,
        outputs, blank_code: blank, force_f64: 0, force_serial: 0, force_generic: 0, max_passes: 0,
    }
}

/// status -> what the reference does in that situation (lib.rs:47-59; the panics of simple/mod.rs:85,103,214)
fn check(st: c_int) -> Result<()> {
    match st {
        0 => Ok(()),
        1 => Err(Error::UnnecessaryArgument),                              // simple/mod.rs:49-51, pwm/mod.rs:36-38
        9 => Err(Error::MatrixShapeError),                                 // pwm/mod.rs:40-42
        2 => panic!("called `Option::unwrap()` on a `None` value"),        // simple/mod.rs:103
        3 => panic!("ndarray: index out of bounds"),                       // simple/mod.rs:85
        4 => panic!("attempt to subtract with overflow"),                  // simple/mod.rs:214
        _ => panic!("aligner_hip: status {st}: {:?}", unsafe { std::ffi::CStr::from_ptr(aln_last_error()) }),
    }
}

fn directions(dirs: Vec<u8>, shape: (usize, usize)) -> Array2<Direction> {
    Array2::from_shape_vec(shape, dirs.into_iter().map(|d| match d {
        0 => Direction::Top, 1 => Direction::Left, 2 => Direction::Diagonal, _ => Direction::Beginning }).collect()).unwrap()
}

macro_rules! hip_aligner { ($name:ident, $sem:expr, $global:expr) => {
pub struct $name<T: BioData + Into<usize> + Copy + Eq> { pub query: Vec<T>, pub target: Vec<T> }

impl<T: BioData + Into<usize> + From<usize> + Copy + Eq> AlignerTrait<T, Alignment<T>> for $name<T> {
    fn from_str_seqs(query: &str, target: &str) -> Result<Self> {
        Ok($name { query: T::str_to_vec(query)?, target: T::str_to_vec(target)? })
    }
    fn from_seqs(query: &[T], target: &[T]) -> Result<Self> {
        Ok($name { query: Vec::from(query), target: Vec::from(target) })
    }
    fn perform_alignment(&mut self, del: f64, ext: f64, matrix: &Array2<f64>, heuristics: Option<Heuristics>)
        -> Result<AlignmentResult<T, Alignment<T>>> {
        let (n, m) = (self.query.len(), self.target.len());
        let want = WANT_MATRICES.load(std::sync::atomic::Ordering::Relaxed);
        let q: Vec<u8> = self.query.iter().map(|r| Into::<usize>::into(*r) as u8).collect();
        let t: Vec<u8> = self.target.iter().map(|r| Into::<usize>::into(*r) as u8).collect();
        let mat = matrix.as_standard_layout().to_owned();          // contiguous rows; row_stride = ncols
        let p = params($sem, del, ext, &mat, heuristics.is_some(),
                       OUT_SCORE | OUT_TRACEBACK | if want { OUT_DIRECTIONS | OUT_H } else { 0 }, Into::<usize>::into(T::blank()) as u8);
        let mut res = AlnPairResult::default();
        let (mut qa, mut ta) = (vec![0u8; n + m + 2], vec![0u8; n + m + 2]);
        let mut dirs = vec![0u8; if want { (n + 1) * (m + 1) } else { 0 }];
        let mut h = if want { Array2::<f64>::zeros((m + 1, n + 1)) } else { Array2::<f64>::zeros((0, 0)) };
        let null = std::ptr::null_mut();
        check(unsafe { aln_align_pair(ctx(), &p, q.as_ptr(), n, t.as_ptr(), m, &mut res, qa.as_mut_ptr(), ta.as_mut_ptr(),
                                      if want { dirs.as_mut_ptr() } else { null }, if want { h.as_mut_ptr() } else { null as *mut f64 }) })?;
        let len = res.aln_len as usize;
        let dec = |v: &[u8]| v[..len].iter().map(|c| T::from(*c as usize)).collect::<Vec<T>>();
        let coords = if $global { ((1, n), (1, m)) }                            // simple/mod.rs:138
            else { ((res.start_x as usize + 1, res.end_x as usize + 1), (res.start_y as usize + 1, res.end_y as usize + 1)) };   // :255-258
        Ok(AlignmentResult { alignment_matrix: h, direction_matrix: directions(dirs, if want { (m + 1, n + 1) } else { (0, 0) }),
            alignment: Alignment { query: dec(&qa), target: dec(&ta), coords, f: res.f },
            matrix: None, phantom: PhantomData })
    }
}}}
hip_aligner!(HipGlobalAligner, CORE_GLOBAL, true);
hip_aligner!(HipLocalAligner, CORE_LOCAL, false);

/// `PWMAligner` (pwm/mod.rs:9-126): `query` are the rows, the columns are the positions of the 4 x W position-weight matrix.
/// The library hands the numbered half of the alignment back as `u32` column numbers (0 = gap, pwm/mod.rs:86-101).
pub struct HipPWMAligner<T: BioData + Into<usize> + Copy + Eq> { pub query: Vec<T> }

impl<T: BioData + Into<usize> + From<usize> + Copy + Eq> AlignerTrait<T, PWMAlignment<T>> for HipPWMAligner<T> {
    fn from_str_seqs(query: &str, _target: &str) -> Result<Self> { Ok(HipPWMAligner { query: T::str_to_vec(query)? }) }     // pwm/mod.rs:14-22
    fn from_seqs(query: &[T], _target: &[T]) -> Result<Self> { Ok(HipPWMAligner { query: Vec::from(query) }) }              // pwm/mod.rs:24-28
    fn perform_alignment(&mut self, del: f64, ext: f64, matrix: &Array2<f64>, heuristics: Option<Heuristics>)
        -> Result<AlignmentResult<T, PWMAlignment<T>>> {
        let (w, m) = (matrix.ncols(), self.query.len());           // dim = (query.len() + 1, W + 1), pwm/mod.rs:46
        let want = WANT_MATRICES.load(std::sync::atomic::Ordering::Relaxed);
        let t: Vec<u8> = self.query.iter().map(|r| Into::<usize>::into(*r) as u8).collect();
        let mat = matrix.as_standard_layout().to_owned();
        let p = params(PWM_LOCAL, del, ext, &mat, heuristics.is_some(),
                       OUT_SCORE | OUT_TRACEBACK | if want { OUT_DIRECTIONS | OUT_H } else { 0 }, Into::<usize>::into(T::blank()) as u8);
        let mut res = AlnPairResult::default();
        let cap = w + m + 2;
        let mut numbered = vec![0u32; cap];                        // q_aln: uint32 column numbers, 4-byte aligned by construction
        let mut qa = vec![0u8; cap];
        let mut dirs = vec![0u8; if want { (w + 1) * (m + 1) } else { 0 }];
        let mut h = if want { Array2::<f64>::zeros((m + 1, w + 1)) } else { Array2::<f64>::zeros((0, 0)) };
        let null = std::ptr::null_mut();
        // (the `query` argument is ignored for ALN_PWM_LOCAL: N = matrix cols)
        check(unsafe { aln_align_pair(ctx(), &p, std::ptr::null(), w, t.as_ptr(), m, &mut res, numbered.as_mut_ptr() as *mut u8, qa.as_mut_ptr(),
                                      if want { dirs.as_mut_ptr() } else { null }, if want { h.as_mut_ptr() } else { null as *mut f64 }) })?;
        let len = res.aln_len as usize;                            // no duplicated seed pair here (pwm/mod.rs:76-103)
        Ok(AlignmentResult { alignment_matrix: h, direction_matrix: directions(dirs, if want { (m + 1, w + 1) } else { (0, 0) }),
            alignment: PWMAlignment {
                numbered: numbered[..len].iter().map(|c| *c as usize).collect(),
                query: qa[..len].iter().map(|c| T::from(*c as usize)).collect(),
                dim: w,                                                                                                // pwm/mod.rs:113
                coords: ((res.start_x as usize + 1, res.end_x as usize + 1), (res.start_y as usize + 1, res.end_y as usize + 1)),   // :114-117
                f: res.f },
            matrix: None, phantom: PhantomData })
    }
}

/// Resident sequence set (`aln_seqset_*`, include/aligner_hip.h): the request path of aligner-web (`generate_pairs`,
/// dispatcher/handlers.rs:253-264) with the residues uploaded once.  A call names a block of the S x S pair grid; `aln_seqset_score`
/// brings back f (and the status) of every pair, `aln_seqset_hits` holds the pairs with f >= f_min -- filled again with directions and
/// walked -- on the device, `aln_seqset_held_list` / `aln_seqset_held_strings` fetch what the caller keeps.
pub mod seqset {
    use super::{AlnCtx, AlnPairResult, AlnParams};
    use std::os::raw::c_int;
    #[repr(C)]
    pub struct AlnSeqset { _private: [u8; 0] }
    #[repr(C)]
    #[derive(Clone, Copy, Default)]
    pub struct AlnSeqsetBlock { pub q_first: u64, pub q_count: u64, pub t_first: u64, pub t_count: u64, pub upper: u32, pub reserved: u32 } // 40 bytes
    impl AlnSeqsetBlock {
        /// every pair i < j of sequences first .. first + n - 1, in generate_pairs order
        pub fn upper(first: u64, n: u64) -> Self { AlnSeqsetBlock { q_first: first, q_count: n, t_first: first, t_count: n, upper: 1, reserved: 0 } }
    }
    pub const ALN_SEQSET_BEST_MAX: u32 = 64;
    pub const ALN_BEST_SKIP_SELF: u32 = 1;
    extern "C" {
        pub fn aln_seqset_create(ctx: *mut AlnCtx, seqs: *const u8, off: *const u64, len: *const u64, n_seqs: usize, status: *mut c_int) -> *mut AlnSeqset;
        pub fn aln_seqset_destroy(set: *mut AlnSeqset);
        pub fn aln_seqset_pairs(set: *const AlnSeqset, block: *const AlnSeqsetBlock) -> u64;
        pub fn aln_seqset_score(set: *mut AlnSeqset, p: *const AlnParams, block: *const AlnSeqsetBlock, f: *mut f64, status: *mut i32) -> c_int;
        pub fn aln_seqset_hits(set: *mut AlnSeqset, p: *const AlnParams, block: *const AlnSeqsetBlock, f_min: f64, count: *mut u64) -> c_int;
        /// the k best targets per query of a rectangle (k in 1 ..= ALN_SEQSET_BEST_MAX), selected on the device and held like the hits
        pub fn aln_seqset_best(set: *mut AlnSeqset, p: *const AlnParams, block: *const AlnSeqsetBlock, k: u32, f_min: f64, flags: u32,
                               count: *mut u64) -> c_int;
        pub fn aln_seqset_held_list(set: *mut AlnSeqset, first: u64, n: u64, pair_index: *mut u64, q_seq: *mut u32, t_seq: *mut u32, f: *mut f64) -> c_int;
        pub fn aln_seqset_held_strings(set: *mut AlnSeqset, keep: *const u32, n_keep: u64, results: *mut AlnPairResult, tb_buf: *mut u8,
                                       tb_off: *const u64) -> c_int;
        pub fn aln_seqset_stats(set: *const AlnSeqset, ms: *mut f64, bytes: *mut u64) -> c_int;
        /// is a held hit better than chance: per listed position one record reduced on the device from `per_pair` shuffled copies of
        /// its target (copy s from the stream (seed, pair_base + the hit's pair index, s)); `f` / `lengths` optional, n_keep * per_pair
        pub fn aln_seqset_held_significance(set: *mut AlnSeqset, p: *const AlnParams, spec: *const AlnShuffleSpec, keep: *const u32, n_keep: u64,
                                            records: *mut AlnSignifRecord, f: *mut f64, lengths: *mut u32) -> c_int;
        /// how identical, how covering, how gapped: the columns of the listed held hits' aligned strings, classed as the midline of
        /// `Alignment::get_alignment` classes them and counted on the device (flags: ALN_REPORT_SKIP_SEED leaves the seed column out)
        pub fn aln_seqset_held_report(set: *mut AlnSeqset, p: *const AlnParams, flags: u32, keep: *const u32, n_keep: u64,
                                      reports: *mut AlnHitReport) -> c_int;
        /// the held positions whose reports pass `filter`, ascending, selected on the device; `reports` optional; `count` is the
        /// number kept in all, also beyond `capacity`
        pub fn aln_seqset_held_filter(set: *mut AlnSeqset, p: *const AlnParams, flags: u32, filter: *const AlnHitFilter, positions: *mut u32,
                                      reports: *mut AlnHitReport, capacity: u64, count: *mut u64) -> c_int;
    }
    pub const ALN_REPORT_SKIP_SEED: u32 = 1;
    /// `aln_hit_report`: the classed columns of one held hit (aligner_amd/csrc/aln_report_rules.h)
    #[repr(C)]
    #[derive(Clone, Copy, Default)]
    pub struct AlnHitReport { pub columns: u32, pub identical: u32, pub positive: u32, pub mismatch: u32, pub q_gap: u32, pub t_gap: u32,
                              pub q_gap_open: u32, pub t_gap_open: u32, pub status: i32, pub reserved: u32 } // 40 bytes
    /// `aln_hit_filter`: kept iff identical >= min_identity * columns, columns - q_gap >= min_q_cover * N, columns - t_gap >=
    /// min_t_cover * M and columns >= min_columns
    #[repr(C)]
    #[derive(Clone, Copy, Default)]
    pub struct AlnHitFilter { pub min_identity: f64, pub min_q_cover: f64, pub min_t_cover: f64, pub min_columns: u32, pub reserved: u32 } // 32 bytes
    /// `aln_shuffle_spec`: the streams of the shuffled copies (aligner_amd/csrc/aln_shuffle_rules.h)
    #[repr(C)]
    #[derive(Clone, Copy, Default)]
    pub struct AlnShuffleSpec { pub seed: u64, pub pair_base: u64, pub per_pair: u32, pub max_trim: u32 } // 24 bytes
    /// `aln_signif_record`: sums in the order of aligner_amd/csrc/aln_signif_rules.h
    #[repr(C)]
    #[derive(Clone, Copy, Default)]
    pub struct AlnSignifRecord { pub sum: f64, pub sum_sq: f64, pub f_max: f64, pub n_ok: u32, pub n_ge: u32, pub status: i32, pub first_bad: u32,
                                 pub reserved: u64 } // 48 bytes
    /// A pair set (`aln_pairset_*`) over pairs first .. first + n_pairs - 1 of a block: it borrows the set's residues.  After
    /// `aln_pairset_heuristics`, `aln_pairset_loop_begin` and one `aln_pairset_loop_step` per iteration run the loop of
    /// HeuristicAligner (heuristic/mod.rs:36-78) for all pairs; a step returns the finished pairs, their causes (0 done, 1 failed,
    /// 2 no root) and summaries, and counts = [run, done, failed, more].
    #[repr(C)]
    pub struct AlnPairset { _private: [u8; 0] }
    extern "C" {
        pub fn aln_pairset_create_from_set(set: *mut AlnSeqset, block: *const AlnSeqsetBlock, first: u64, n_pairs: u64, status: *mut c_int) -> *mut AlnPairset;
        pub fn aln_pairset_loop_begin(ps: *mut AlnPairset, shared_matrix: *const f64, status: *mut i32) -> c_int;
        pub fn aln_pairset_loop_step(ps: *mut AlnPairset, p: *const AlnParams, finished: *mut u32, cause: *mut u32,
                                     finished_results: *mut AlnPairResult, counts: *mut u32) -> c_int;
    }
}

/// The batch site of the reference, `calculate_p_value` (statistics/mod.rs:255-286): one query against `targets.len()` shuffled
/// targets, only `alignment.f` is kept.  One call instead of ten threads x 500 aligners; `del` / `ins` / `matrix` as there.
pub fn local_scores<T: BioData + Into<usize> + Copy + Eq>(query: &[T], targets: &[Vec<T>], del: f64, ins: f64, matrix: &Array2<f64>) -> Vec<f64> {
    let mut seqs: Vec<u8> = query.iter().map(|r| Into::<usize>::into(*r) as u8).collect();        // offset 0: the query, shared by every pair
    let (mut t_off, mut t_len) = (Vec::with_capacity(targets.len()), Vec::with_capacity(targets.len()));
    for t in targets {
        t_off.push(seqs.len() as u64);
        t_len.push(t.len() as u64);
        seqs.extend(t.iter().map(|r| Into::<usize>::into(*r) as u8));
    }
    let (q_off, q_len) = (vec![0u64; targets.len()], vec![query.len() as u64; targets.len()]);
    let mut results = vec![AlnPairResult::default(); targets.len()];
    let mat = matrix.as_standard_layout().to_owned();
    let p = params(CORE_LOCAL, del, ins, &mat, false, OUT_SCORE, Into::<usize>::into(T::blank()) as u8);
    let st = unsafe { aln_align_batch(ctx(), &p, seqs.as_ptr(), q_off.as_ptr(), q_len.as_ptr(), t_off.as_ptr(), t_len.as_ptr(), targets.len(),
                                      results.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null()) };
    check(st).expect("aligner_hip batch call");
    results.iter().map(|r| { check(r.status).expect("aligner_hip pair"); r.f }).collect()         // what :273-279 kept
}
