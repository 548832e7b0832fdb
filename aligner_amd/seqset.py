"""A set of sequences resident in HBM, scored all against all (aln_seqset_*, include/aligner_hip.h).

The device-resident form of the reference's request path (generate_pairs, aligner-web/src/bin/dispatcher/handlers.rs:253-264:
every pair i < j of a FASTA): the residues go up once, a call names a block of the S x S pair grid, and either every pair's f or
the held hits -- the pairs at or above a threshold, filled again with directions and walked -- come back.  Sequence q of a pair is
the query (columns), sequence t the target (rows); pair k of a block is what align_batch computes for (q, t).
"""
import ctypes as C

import numpy as np

from . import _ffi
from . import runtime
from . import statistics
from .alignment import Alignment
from .batch import RESULT_DTYPE
from .enums import Protein


# aln_signif_record (include/aligner_hip.h) and what HeldHits.significance makes of it
SIGNIF_RECORD_DTYPE = np.dtype([("sum", "<f8"), ("sum_sq", "<f8"), ("f_max", "<f8"), ("n_ok", "<u4"), ("n_ge", "<u4"), ("status", "<i4"),
                                ("first_bad", "<u4"), ("reserved", "<u8")])
SIGNIF_DTYPE = np.dtype([("mean", "<f8"), ("sd", "<f8"), ("z", "<f8"), ("p_emp", "<f8"), ("n_ok", "<u4"), ("status", "<i4")])
assert SIGNIF_RECORD_DTYPE.itemsize == 48
# aln_hit_report (include/aligner_hip.h) and what report_fractions makes of it
REPORT_DTYPE = np.dtype([("columns", "<u4"), ("identical", "<u4"), ("positive", "<u4"), ("mismatch", "<u4"), ("q_gap", "<u4"), ("t_gap", "<u4"),
                         ("q_gap_open", "<u4"), ("t_gap_open", "<u4"), ("status", "<i4"), ("reserved", "<u4")])
FRACTIONS_DTYPE = np.dtype([("identity", "<f8"), ("positives", "<f8"), ("q_cover", "<f8"), ("t_cover", "<f8"), ("gap_opens", "<u4"),
                            ("gaps", "<u4")])
assert REPORT_DTYPE.itemsize == 40


def report_fractions(reports, q_len, t_len):
    """What a user asks of a hit, out of its report and the lengths N, M of its query and target sequences: identity = identical /
    columns, positives = (identical + positive) / columns, q_cover = (columns - q_gap) / N, t_cover = (columns - t_gap) / M,
    gap_opens = q_gap_open + t_gap_open, gaps = q_gap + t_gap.  0 / 0 is NaN; nothing is raised or warned about."""
    reports = np.asarray(reports, dtype=REPORT_DTYPE)
    out = np.zeros(len(reports), dtype=FRACTIONS_DTYPE)
    with np.errstate(all="ignore"):
        cols = reports["columns"].astype(np.float64)
        out["identity"] = reports["identical"].astype(np.float64) / cols
        out["positives"] = (reports["identical"].astype(np.float64) + reports["positive"].astype(np.float64)) / cols
        out["q_cover"] = (cols - reports["q_gap"].astype(np.float64)) / np.asarray(q_len, dtype=np.float64)
        out["t_cover"] = (cols - reports["t_gap"].astype(np.float64)) / np.asarray(t_len, dtype=np.float64)
    out["gap_opens"] = reports["q_gap_open"] + reports["t_gap_open"]
    out["gaps"] = reports["q_gap"] + reports["t_gap"]
    return out


def significance_from_records(records, f_hit):
    """mean, sd, z and the empirical p of hits with score f_hit out of their records: mean = sum / n_ok, sd = sqrt(sum_sq / n_ok -
    mean^2) clamped at 0 (the population form, as calculate_starting_values of the repeat search, engine/calc.rs:76-84),
    z = (f - mean) / sd, p_emp = (n_ge + 1) / (n_ok + 1).  No copy succeeded: mean, sd and z are NaN, p_emp is 1; sd = 0: z is +-inf
    or NaN.  Nothing is raised or warned about."""
    records = np.asarray(records, dtype=SIGNIF_RECORD_DTYPE)
    f_hit = np.asarray(f_hit, dtype=np.float64)
    out = np.zeros(len(records), dtype=SIGNIF_DTYPE)
    with np.errstate(all="ignore"):
        n = records["n_ok"].astype(np.float64)
        mean = records["sum"] / n
        var = records["sum_sq"] / n - mean * mean
        sd = np.sqrt(np.where(var < 0.0, 0.0, var))
        out["mean"], out["sd"] = mean, sd
        out["z"] = (f_hit - mean) / sd
        out["p_emp"] = (records["n_ge"].astype(np.float64) + 1.0) / (n + 1.0)
    out["n_ok"], out["status"] = records["n_ok"], records["status"]
    return out


def _block(block, n):
    """A block as the C struct: a SeqsetBlock, None (the upper triangle of the whole set), or a dict / tuple
    (q_first, q_count, t_first, t_count[, upper])."""
    if isinstance(block, _ffi.SeqsetBlock):
        return block
    if block is None:
        return _ffi.SeqsetBlock(0, n, 0, n, 1, 0)
    if isinstance(block, dict):
        return _ffi.SeqsetBlock(int(block["q_first"]), int(block["q_count"]), int(block["t_first"]), int(block["t_count"]),
                                int(block.get("upper", 0)), int(block.get("reserved", 0)))
    b = tuple(block)
    return _ffi.SeqsetBlock(int(b[0]), int(b[1]), int(b[2]), int(b[3]), int(b[4]) if len(b) > 4 else 0, 0)


def upper(first, count):
    """The pairs i < j of sequences first .. first + count - 1, in generate_pairs order."""
    return _ffi.SeqsetBlock(int(first), int(count), int(first), int(count), 1, 0)


def rectangle(q_first, q_count, t_first, t_count):
    """Every (q, t) with q in the first range and t in the second; the queries are the slow index."""
    return _ffi.SeqsetBlock(int(q_first), int(q_count), int(t_first), int(t_count), 0, 0)


def minus(block, n):
    """The same rectangle of a stranded set of n records on the minus strand: the targets shifted onto their mirrors."""
    if block.upper:
        raise ValueError("seqset.minus: a rectangle, not an upper block")
    return _ffi.SeqsetBlock(block.q_first, block.q_count, block.t_first + int(n), block.t_count, 0, 0)


def both(block, n):
    """The rectangle of a stranded set of n records that holds every query of `block` against all its targets on both strands: the
    target range widened to 0 .. 2n - 1 when it is the whole 0 .. n - 1 (only then is the union one rectangle)."""
    if block.upper or block.t_first != 0 or block.t_count != int(n):
        raise ValueError("seqset.both: a rectangle whose targets are all n records")
    return _ffi.SeqsetBlock(block.q_first, block.q_count, 0, 2 * int(n), 0, 0)


def window(block, first, n):
    """(q, t) uint64 arrays: the sequence numbers of pairs first .. first + n - 1 of a valid block, in the numbering of
    aligner_amd/csrc/aln_seqset_rules.h, with numpy on whole arrays (exact: integers below 2^63)."""
    k = np.arange(int(first), int(first) + int(n), dtype=np.int64)
    if not block.upper:
        return (block.q_first + k // block.t_count).astype(np.uint64), (block.t_first + k % block.t_count).astype(np.uint64)
    m = int(block.q_count)
    r = np.arange(m, dtype=np.int64)
    start = r * (m - 1) - r * (r - 1) // 2                                      # the pairs in front of row r
    row = np.searchsorted(start[:max(m - 1, 1)], k, side="right") - 1
    return (block.q_first + row).astype(np.uint64), (block.q_first + row + 1 + (k - start[row])).astype(np.uint64)


class SeqSet:
    def __init__(self, seqs, alphabet=Protein, device=None, _map=None):
        """seqs: residue code arrays (or strings, encoded with alphabet.str_to_vec)."""
        self.lib = _ffi.load()
        self.alphabet = alphabet
        codes = [np.asarray(alphabet.str_to_vec(s) if isinstance(s, str) else s, dtype=np.uint8) for s in seqs]
        self.len = np.array([len(c) for c in codes], dtype=np.uint64)
        self.off = np.zeros(len(codes), dtype=np.uint64)
        if len(codes) > 1:
            self.off[1:] = np.cumsum(self.len)[:-1]
        self.seqs = np.concatenate(codes) if codes else np.zeros(0, dtype=np.uint8)
        st = C.c_int(0)
        self.records = len(codes)              # the caller's records: of a stranded set half of len()
        self.map = None
        if _map is None:
            self.handle = self.lib.aln_seqset_create(runtime.context(device), self.seqs.ctypes.data, self.off.ctypes.data, self.len.ctypes.data,
                                                     len(codes), C.byref(st))
        else:
            # the host's view of the 2n resident records: lengths and offsets as the device lays them out; only the n forward records
            # go up, and .seqs gains the mirrors, made here in numpy, when it is first asked for
            self.map = np.ascontiguousarray(_map, dtype=np.uint8)
            if self.map.shape != (256,):
                raise ValueError("SeqSet.stranded: map is a table of 256 bytes")
            self.handle = self.lib.aln_seqset_create_stranded(runtime.context(device), self.seqs.ctypes.data, self.off.ctypes.data,
                                                              self.len.ctypes.data, len(codes), self.map.ctypes.data, C.byref(st))
            total = len(self._seqs)
            self._forward, self._seqs = codes, None
            self.off = np.concatenate([self.off, self.off + np.uint64(total)]).astype(np.uint64)
            self.len = np.concatenate([self.len, self.len])
        if not self.handle:
            runtime.raise_for_status(st.value, "aln_seqset_create_stranded" if _map is not None else "aln_seqset_create")
            raise RuntimeError("aln_seqset_create returned NULL")
        self._word = None          # the (k, alphabet_size) of the word index this object built (word_index), if any

    @classmethod
    def stranded(cls, seqs, alphabet=None, device=None, map=None):
        """aln_seqset_create_stranded: the n records and, made on the device behind them, their n mirrors -- record n + i is
        map[record i reversed] -- as one set of 2n resident records that every other call takes as ordinary records.  map: 256 bytes
        (default: alphabet.complement_map(), alphabet DNA unless given).  .records is n, len() is 2n; minus() and both() shift and
        widen a rectangle onto the mirrors."""
        from .enums import DNA
        alphabet = DNA if alphabet is None else alphabet
        return cls(seqs, alphabet, device=device, _map=alphabet.complement_map() if map is None else map)

    @property
    def is_stranded(self):
        return self.map is not None

    @property
    def seqs(self):
        """The residues of every resident record, packed as the device holds them (of a stranded set the mirrors are made on the host
        the first time this is read; residues() brings down what the device made)."""
        if self._seqs is None:
            self._seqs = np.concatenate(self._forward + [self.map[c[::-1]] for c in self._forward]) if self._forward else np.zeros(0, dtype=np.uint8)
        return self._seqs

    @seqs.setter
    def seqs(self, value):
        self._seqs = value

    def residues(self, first=0, count=None):
        """aln_seqset_strand_residues: resident records first .. first + count - 1 (default: to the last) as the device holds them, a
        list of uint8 arrays."""
        count = len(self) - int(first) if count is None else int(count)
        lens = self.len[int(first):int(first) + count]
        off = np.zeros(count, dtype=np.uint64)
        if count > 1:
            off[1:] = np.cumsum(lens)[:-1]
        out = np.zeros(max(int(lens.sum()), 1), dtype=np.uint8)
        st = self.lib.aln_seqset_strand_residues(self.handle, int(first), count, off.ctypes.data, out.ctypes.data)
        runtime.raise_for_status(st, "aln_seqset_strand_residues")
        return [out[int(a):int(a) + int(n)].copy() for a, n in zip(off, lens)]

    def __len__(self):
        return len(self.len)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.handle:
            self.lib.aln_seqset_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pairs(self, block=None):
        """Pairs of a block; 0 for an invalid one."""
        b = _block(block, len(self))
        return int(self.lib.aln_seqset_pairs(self.handle, C.byref(b)))

    def _checked(self, block):
        b = _block(block, len(self))
        n = int(self.lib.aln_seqset_pairs(self.handle, C.byref(b)))
        if n == 0:
            raise ValueError("aln_seqset: invalid block (a range beyond the set, unequal ranges of an upper block, or no pairs)")
        return b, n

    def score(self, matrix, del_, ext, block=None, semantics=_ffi.CORE_LOCAL, blank=98, **kw):
        """(f, status) of every pair of the block: f64 and int32 arrays in the block's pair order.  A failed pair carries its status
        (its f is 0) and leaves the others untouched."""
        b, n = self._checked(block)
        p, keep = runtime.make_params(semantics, del_, ext, matrix, outputs=_ffi.OUT_SCORE, blank=blank, **kw)
        f = np.zeros(n, dtype=np.float64)
        status = np.zeros(n, dtype=np.int32)
        st = self.lib.aln_seqset_score(self.handle, C.byref(p), C.byref(b), f.ctypes.data, status.ctypes.data)
        runtime.raise_for_status(st, "aln_seqset_score")
        return f, status

    def hits(self, matrix, del_, ext, f_min, block=None, semantics=_ffi.CORE_LOCAL, blank=98, **kw):
        """A held pass: the pairs with f >= f_min, aligned.  Returns a HeldHits (valid until the next score / hits on this set)."""
        b, n = self._checked(block)
        p, keep = runtime.make_params(semantics, del_, ext, matrix, blank=blank, **kw)
        count = C.c_uint64(0)
        st = self.lib.aln_seqset_hits(self.handle, C.byref(p), C.byref(b), float(f_min), C.byref(count))
        runtime.raise_for_status(st, "aln_seqset_hits")
        return HeldHits(self, int(count.value), semantics)

    def best(self, matrix, del_, ext, k, f_min=float("-inf"), block=None, skip_self=False, semantics=_ffi.CORE_LOCAL, blank=98, **kw):
        """A held pass: of every query of a rectangle (default: the whole set against itself) the k best targets among the pairs that
        succeeded with f >= f_min -- higher f first, equal f by the lower target number -- selected on the device and aligned.
        skip_self leaves (i, i) out.  Returns a BestHits (valid until the next score / hits / best on this set)."""
        if block is None:
            block = rectangle(0, len(self), 0, len(self))
        b, n = self._checked(block)
        p, keep = runtime.make_params(semantics, del_, ext, matrix, blank=blank, **kw)
        count = C.c_uint64(0)
        st = self.lib.aln_seqset_best(self.handle, C.byref(p), C.byref(b), int(k), float(f_min), _ffi.BEST_SKIP_SELF if skip_self else 0,
                                      C.byref(count))
        runtime.raise_for_status(st, "aln_seqset_best")
        return BestHits(self, int(count.value), semantics)

    def kmer_index(self, k, alphabet_size):
        """aln_seqset_kmer_index: builds (or replaces) the resident k-mer bitmaps -- words of k residues with every code below
        alphabet_size, alphabet_size ** k <= 2 ** 18 -- and returns n(s), the number of distinct words, of every sequence (uint32).
        Any candidate list is dropped."""
        n_words = np.zeros(len(self), dtype=np.uint32)
        st = self.lib.aln_seqset_kmer_index(self.handle, int(k), int(alphabet_size), n_words.ctypes.data)
        runtime.raise_for_status(st, "aln_seqset_kmer_index")
        self._kmer = (int(k), int(alphabet_size))
        return n_words

    def prefilter(self, k, alphabet_size, min_shared=0, min_per_1024=0, block=None, chunk_pairs=0):
        """aln_seqset_prefilter: the pairs of the block whose sequences share at least min_shared distinct words, and at least
        min_per_1024 / 1024 of the smaller of their two word counts (integer rule: aligner_amd/csrc/aln_prefilter_rules.h), selected
        on the device.  Builds the index if none of this (k, alphabet_size) is there.  Returns a Candidates (valid until the next
        kmer_index / prefilter on this set; score, hits and best leave it alone)."""
        b, n = self._checked(block)
        if getattr(self, "_kmer", None) != (int(k), int(alphabet_size)):
            self.kmer_index(k, alphabet_size)
        spec = _ffi.PrefilterSpec(int(k), int(alphabet_size), int(min_shared), int(min_per_1024), int(chunk_pairs), 0, 0)
        count = C.c_uint64(0)
        st = self.lib.aln_seqset_prefilter(self.handle, C.byref(spec), C.byref(b), C.byref(count))
        runtime.raise_for_status(st, "aln_seqset_prefilter")
        return Candidates(self, int(count.value))

    def word_index(self, k, alphabet_size):
        """aln_seqset_word_index: builds (or replaces) the resident sorted list of the distinct (word, sequence) of the set -- words of
        k residues with every code below alphabet_size, alphabet_size ** k <= 2 ** 32 -- and returns n(s), the number of distinct
        words, of every sequence (uint32): what kmer_index returns where both build.  Any candidate list is dropped; the bitmaps of
        kmer_index stay."""
        n_words = np.zeros(len(self), dtype=np.uint32)
        st = self.lib.aln_seqset_word_index(self.handle, int(k), int(alphabet_size), n_words.ctypes.data)
        runtime.raise_for_status(st, "aln_seqset_word_index")
        self._word = (int(k), int(alphabet_size))
        return n_words

    def word_join(self, k, alphabet_size, min_shared=1, min_per_1024=0, block=None, chunk_occurrences=0):
        """aln_seqset_word_join: the candidates of prefilter(k, alphabet_size, min_shared, min_per_1024, block) with min_shared >= 1,
        the same list entry for entry, by a join over the posting lists of the sorted word index: work follows what the sequences
        share, not the number of pairs.  Builds the word index if none of this (k, alphabet_size) is there.  Returns a Candidates."""
        b, n = self._checked(block)
        if self._word != (int(k), int(alphabet_size)):
            self.word_index(k, alphabet_size)
        spec = _ffi.WordjoinSpec(int(k), int(alphabet_size), int(min_shared), int(min_per_1024), int(chunk_occurrences), 0, 0)
        count = C.c_uint64(0)
        st = self.lib.aln_seqset_word_join(self.handle, C.byref(spec), C.byref(b), C.byref(count))
        runtime.raise_for_status(st, "aln_seqset_word_join")
        return Candidates(self, int(count.value))

    def seed_index(self, k, alphabet_size):
        """aln_seqset_seed_index: builds (or replaces) the resident list of every occurrence (word, sequence, position) of the set --
        words of k residues, k up to 16, with every code below alphabet_size, alphabet_size ** k <= 2 ** 32 -- and returns how many
        there are.  Any candidate list is dropped; the bitmaps of kmer_index and the list of word_index stay."""
        occurrences = C.c_uint64(0)
        st = self.lib.aln_seqset_seed_index(self.handle, int(k), int(alphabet_size), C.byref(occurrences))
        runtime.raise_for_status(st, "aln_seqset_seed_index")
        self._seed = (int(k), int(alphabet_size))
        return int(occurrences.value)

    def seed_join(self, k, alphabet_size, min_seeds=1, band=0, max_occ=0, block=None, chunk_seeds=0):
        """aln_seqset_seed_join: the pairs of the block with at least min_seeds seeds -- word hits (pq, pt), diagonal pt - pq -- on
        diagonals d0 .. d0 + band for some d0, words with more than max_occ occurrences in the whole set left out (0: none).  Builds
        the seed index if none of this (k, alphabet_size) is there.  Returns a Candidates whose .shared holds the seeds of the best
        band, .diag its least diagonal d0 and .summary the call's counts; on a mirrored record of a stranded set the diagonal is in the
        mirror's coordinates."""
        b, n = self._checked(block)
        if getattr(self, "_seed", None) != (int(k), int(alphabet_size)):
            self.seed_index(k, alphabet_size)
        spec = _ffi.SeedjoinSpec(int(k), int(alphabet_size), int(min_seeds), int(band), int(max_occ), int(chunk_seeds), 0, 0)
        summ = _ffi.SeedjoinSummary()
        count = C.c_uint64(0)
        st = self.lib.aln_seqset_seed_join(self.handle, C.byref(spec), C.byref(b), C.byref(summ), C.byref(count))
        runtime.raise_for_status(st, "aln_seqset_seed_join")
        return Candidates(self, int(count.value), diags=True,
                          summary=dict(seeds=int(summ.seeds), pairs_with_seed=int(summ.pairs_with_seed), words_dropped=int(summ.words_dropped),
                                       chunks=int(summ.chunks)), seed=(int(k), int(alphabet_size)))

    def stats(self):
        """(after best, fetch_kernel_ms is the selection kernels' time until a held fetch overwrites it; after kmer_index and
        prefilter it is the index and sharing kernels' time)"""
        ms, by = (C.c_double * 4)(), (C.c_uint64 * 2)()
        runtime.raise_for_status(self.lib.aln_seqset_stats(self.handle, ms, by), "aln_seqset_stats")
        return dict(fill_ms=ms[0], refill_ms=ms[1], fetch_kernel_ms=ms[2], wall_ms=ms[3], bytes_up=int(by[0]), bytes_down=int(by[1]))


# aln_chain_record (include/aligner_hip_seedchain.h)
CHAIN_RECORD = np.dtype([("score", "<i4"), ("anchors", "<u4"), ("q_start", "<u4"), ("q_end", "<u4"), ("t_start", "<u4"), ("t_end", "<u4"),
                         ("seeds", "<u4"), ("flags", "<u4")])


def _chain_summary(summ):
    return dict(anchors=int(summ.anchors), with_anchor=int(summ.with_anchor), overflowed=int(summ.overflowed), chunks=int(summ.chunks))


class Candidates:
    """The candidate list of SeqSet.prefilter: .index (pair numbers in the block), .q, .t (sequence numbers) and .shared (distinct
    words both sequences hold) in ascending pair order.  .score(...) aligns the candidates only, .hits(...) holds those at or above
    a threshold as SeqSet.hits would, .best(...) the k best of every query's candidates as SeqSet.best would.  A list of
    SeqSet.seed_join holds the seeds of the pair's best band in .shared, and has .diag (int32, the band's least diagonal) and .summary;
    on the other routes both are None.  .chains(...) gives every candidate's seed chain (CHAIN_RECORD), .chain_filter(...) the list
    of those whose chain is good enough, which carries the kept records in .chain.  .chain_summary is None until .chains has run, then
    the counts of its last call (anchors, with_anchor, overflowed, chunks)."""

    def __init__(self, owner, count, diags=False, summary=None, seed=None, chain=False):
        self.owner, self.count = owner, count
        self.diag, self.summary, self.chain, self.chain_summary = None, summary, None, None
        self._seed = seed                 # (k, alphabet_size) of the seed index a seed-join list was made from
        if chain:
            self.chain = np.zeros(count, dtype=CHAIN_RECORD)
            if count:
                st = owner.lib.aln_seqset_candidate_chain_records(owner.handle, 0, count, self.chain.ctypes.data)
                runtime.raise_for_status(st, "aln_seqset_candidate_chain_records")
        if diags:
            self.diag = np.zeros(count, dtype=np.int32)
            if count:
                st = owner.lib.aln_seqset_candidate_diags(owner.handle, 0, count, self.diag.ctypes.data)
                runtime.raise_for_status(st, "aln_seqset_candidate_diags")
        self.index = np.zeros(count, dtype=np.uint64)
        self.q = np.zeros(count, dtype=np.uint32)
        self.t = np.zeros(count, dtype=np.uint32)
        self.shared = np.zeros(count, dtype=np.uint32)
        if count:
            st = owner.lib.aln_seqset_candidates(owner.handle, 0, count, self.index.ctypes.data, self.q.ctypes.data, self.t.ctypes.data,
                                                 self.shared.ctypes.data)
            runtime.raise_for_status(st, "aln_seqset_candidates")

    def __len__(self):
        return self.count

    def _chain_spec(self, max_gap, max_skew, gap_scale, max_occ, max_pair_seeds, chunk_anchors, k, alphabet_size):
        """the spec of a chaining call.  The set's seed index must be of (k, alphabet_size): it is built here only while the list is
        empty, since building an index drops the list; otherwise ValueError asks for seed_index before the list is made"""
        if k is None and alphabet_size is None and self._seed is not None:
            k, alphabet_size = self._seed
        if k is None or alphabet_size is None:
            raise TypeError("a list of prefilter or word_join names no seed index: give k= and alphabet_size=")
        o = self.owner
        if getattr(o, "_seed", None) != (int(k), int(alphabet_size)):
            if self.count:
                raise ValueError("the set's seed index is not of (k, alphabet_size) = (%d, %d) and building it would drop this list: "
                                 "call seed_index before the list is made" % (int(k), int(alphabet_size)))
            o.seed_index(k, alphabet_size)
        return _ffi.SeedchainSpec(int(k), int(alphabet_size), int(max_occ), int(max_gap), int(max_skew), int(gap_scale), int(max_pair_seeds),
                                  int(chunk_anchors), 0, (C.c_uint32 * 3)(0, 0, 0))

    def chains(self, max_gap=1000, max_skew=200, gap_scale=2, max_occ=0, max_pair_seeds=0, chunk_anchors=0, k=None, alphabet_size=None):
        """aln_seqset_candidate_chains: the colinear chain over all seeds (anchors) of every candidate, on the device, as a structured
        array (CHAIN_RECORD: score, anchors, q_start, q_end, t_start, t_end, seeds, flags) in list order.  An anchor may follow another
        within max_gap on both records and max_skew of diagonal drift; a link gains min(the two distances, k) and costs
        (drift * gap_scale) >> 4; the chain ends at the best anchor, the ends are half open.  A candidate with more than
        max_pair_seeds anchors (0: 2 ** 16) is not chained: flags = CHAIN_OVERFLOW, seeds = its anchors.  The list stays as it is.  On
        a list of prefilter or word_join, k and alphabet_size name the seed index and are required.  The seed index of that (k,
        alphabet_size) must already be there: building one drops the candidate list, so on a list that is not empty this raises
        ValueError instead of building it (call SeqSet.seed_index before the list is made; a seed_join list always has its index).
        The call's counts (anchors, with_anchor, overflowed, chunks) are left in .chain_summary."""
        spec = self._chain_spec(max_gap, max_skew, gap_scale, max_occ, max_pair_seeds, chunk_anchors, k, alphabet_size)
        out = np.zeros(self.count, dtype=CHAIN_RECORD)
        summ = _ffi.SeedchainSummary()
        o = self.owner
        st = o.lib.aln_seqset_candidate_chains(o.handle, C.byref(spec), 0, self.count, out.ctypes.data if self.count else None, C.byref(summ))
        runtime.raise_for_status(st, "aln_seqset_candidate_chains")
        self.chain_summary = _chain_summary(summ)
        return out

    def chain_filter(self, min_score, min_span=0, max_gap=1000, max_skew=200, gap_scale=2, max_occ=0, max_pair_seeds=0, chunk_anchors=0, k=None,
                     alphabet_size=None):
        """aln_seqset_candidate_chain_filter: replaces the set's candidate list with the candidates that overflowed or whose chain has
        score >= min_score and spans at least min_span on both records, in their order.  Returns the new Candidates: .chain holds the
        kept records, .summary the call's counts, .diag is carried over.  This object is stale afterwards, as after any call that
        replaces the list (kmer_index / prefilter / word_join / seed_join).  As with chains, the seed index of (k, alphabet_size) must
        already be there: ValueError on a list that is not empty otherwise, since building the index would drop the list."""
        spec = self._chain_spec(max_gap, max_skew, gap_scale, max_occ, max_pair_seeds, chunk_anchors, k, alphabet_size)
        summ = _ffi.SeedchainSummary()
        count = C.c_uint64(0)
        o = self.owner
        st = o.lib.aln_seqset_candidate_chain_filter(o.handle, C.byref(spec), int(min_score), int(min_span), C.byref(summ), C.byref(count))
        runtime.raise_for_status(st, "aln_seqset_candidate_chain_filter")
        return Candidates(o, int(count.value), diags=self.diag is not None, summary=_chain_summary(summ), seed=(int(spec.k), int(spec.alphabet)),
                          chain=True)

    def score(self, matrix, del_, ext, semantics=_ffi.CORE_LOCAL, blank=98, **kw):
        """(f, status) of every candidate, in list order: what SeqSet.score gives for those pairs, bit for bit."""
        o = self.owner
        p, keep = runtime.make_params(semantics, del_, ext, matrix, outputs=_ffi.OUT_SCORE, blank=blank, **kw)
        f = np.zeros(self.count, dtype=np.float64)
        status = np.zeros(self.count, dtype=np.int32)
        st = o.lib.aln_seqset_candidate_scores(o.handle, C.byref(p), f.ctypes.data, status.ctypes.data)
        runtime.raise_for_status(st, "aln_seqset_candidate_scores")
        return f, status

    def hits(self, matrix, del_, ext, f_min, semantics=_ffi.CORE_LOCAL, blank=98, **kw):
        """A held pass over the candidates: those with f >= f_min, aligned.  Returns a HeldHits whose .index are pair numbers of
        the prefilter's block."""
        o = self.owner
        p, keep = runtime.make_params(semantics, del_, ext, matrix, blank=blank, **kw)
        count = C.c_uint64(0)
        st = o.lib.aln_seqset_candidate_hits(o.handle, C.byref(p), float(f_min), C.byref(count))
        runtime.raise_for_status(st, "aln_seqset_candidate_hits")
        return HeldHits(o, int(count.value), semantics)

    def best(self, matrix, del_, ext, k, f_min=float("-inf"), skip_self=False, semantics=_ffi.CORE_LOCAL, blank=98, **kw):
        """A held pass over the candidates: of every query of the prefilter's rectangle the k best targets among its candidates that
        succeeded with f >= f_min -- higher f first, equal f by the lower target number -- selected on the device and aligned.
        skip_self leaves a listed (i, i) out (it is aligned, then skipped).  Returns a BestHits whose .index are pair numbers of the
        prefilter's block; the candidate list stays."""
        o = self.owner
        p, keep = runtime.make_params(semantics, del_, ext, matrix, blank=blank, **kw)
        count = C.c_uint64(0)
        st = o.lib.aln_seqset_candidate_best(o.handle, C.byref(p), int(k), float(f_min), _ffi.BEST_SKIP_SELF if skip_self else 0,
                                             C.byref(count))
        runtime.raise_for_status(st, "aln_seqset_candidate_best")
        return BestHits(o, int(count.value), semantics)


class HeldHits:
    """The hits of SeqSet.hits: .index (pair numbers in the block), .q, .t (sequence numbers) and .f in ascending pair order;
    .alignments(keep) fetches Alignment objects of the listed positions."""

    def __init__(self, owner, count, semantics):
        self.owner, self.count, self.semantics = owner, count, semantics
        self.index = np.zeros(count, dtype=np.uint64)
        self.q = np.zeros(count, dtype=np.uint32)
        self.t = np.zeros(count, dtype=np.uint32)
        self.f = np.zeros(count, dtype=np.float64)
        if count:
            st = owner.lib.aln_seqset_held_list(owner.handle, 0, count, self.index.ctypes.data, self.q.ctypes.data, self.t.ctypes.data,
                                                self.f.ctypes.data)
            runtime.raise_for_status(st, "aln_seqset_held_list")

    def __len__(self):
        return self.count

    def strings(self, keep=None):
        """(summaries, [(aligned query, aligned target)]) of the listed positions of the held list (default: all)."""
        o = self.owner
        w = np.arange(self.count, dtype=np.uint32) if keep is None else np.ascontiguousarray(keep, dtype=np.uint32)
        if len(w) and int(w.max()) >= self.count:
            raise ValueError("aln_seqset_held_strings: a listed position is beyond the held hits")
        cap = (o.len[self.q[w]] + o.len[self.t[w]] + np.uint64(2)).astype(np.uint64) if len(w) else np.zeros(0, dtype=np.uint64)
        off = np.zeros(len(w), dtype=np.uint64)
        if len(w) > 1:
            off[1:] = np.cumsum(2 * cap)[:-1]
        tb = np.zeros(max(int((2 * cap).sum()), 1), dtype=np.uint8)
        res = np.zeros(len(w), dtype=RESULT_DTYPE)
        st = o.lib.aln_seqset_held_strings(o.handle, w.ctypes.data, len(w), res.ctypes.data, tb.ctypes.data, off.ctypes.data)
        runtime.raise_for_status(st, "aln_seqset_held_strings")
        out = []
        for k in range(len(w)):
            n = int(res["aln_len"][k]) if res["status"][k] == _ffi.OK else 0
            a, c = int(off[k]), int(cap[k])
            out.append((tb[a:a + n].copy(), tb[a + c:a + c + n].copy()))
        return res, out

    def _keep(self, keep):
        return np.arange(self.count, dtype=np.uint32) if keep is None else np.ascontiguousarray(keep, dtype=np.uint32)

    def significance_records(self, matrix, del_, ext, seed, per_pair=statistics.SEQUENCES - 1, max_trim=6, keep=None, pair_base=0, scores=False,
                             semantics=None, blank=98, **kw):
        """aln_seqset_held_significance: (records, f, lengths) of the listed positions of the held list (default: all) -- the 48-byte
        records as SIGNIF_RECORD_DTYPE, and with scores=True f float64[n, per_pair] and lengths uint32[n, per_pair] of every copy
        (None otherwise).  Copy s of a hit comes from the stream (seed, pair_base + its .index, s).  semantics: the held pass's unless
        given."""
        o = self.owner
        w = self._keep(keep)
        if not 1 <= int(per_pair) <= _ffi.SHUFFLE_MAX_COPIES:          # (before the per-copy arrays are sized by it)
            raise ValueError("aln_seqset_held_significance: per_pair must lie in 1 .. %d" % _ffi.SHUFFLE_MAX_COPIES)
        p, _held = runtime.make_params(self.semantics if semantics is None else semantics, del_, ext, matrix, outputs=_ffi.OUT_SCORE,
                                       blank=blank, **kw)
        spec = _ffi.ShuffleSpec(int(seed) & 0xFFFFFFFFFFFFFFFF, int(pair_base) & 0xFFFFFFFFFFFFFFFF, int(per_pair), int(max_trim))
        rec = np.zeros(len(w), dtype=SIGNIF_RECORD_DTYPE)
        shape = (len(w), int(per_pair)) if scores else None
        f = np.zeros(shape, dtype=np.float64) if scores else None
        lengths = np.zeros(shape, dtype=np.uint32) if scores else None
        st = o.lib.aln_seqset_held_significance(o.handle, C.byref(p), C.byref(spec), w.ctypes.data, len(w), rec.ctypes.data,
                                                f.ctypes.data if scores else None, lengths.ctypes.data if scores else None)
        runtime.raise_for_status(st, "aln_seqset_held_significance")
        return rec, f, lengths

    def significance(self, matrix, del_, ext, seed, per_pair=statistics.SEQUENCES - 1, max_trim=6, keep=None, pair_base=0, scores=False, **kw):
        """Is a held hit better than chance?  Every listed hit's query against per_pair trimmed and shuffled copies of its target,
        drawn, scored and reduced on the device.  Returns a SIGNIF_DTYPE array (mean, sd, z, p_emp, n_ok, status: see
        significance_from_records); with scores=True (that, f, lengths) of every copy as well."""
        w = self._keep(keep)
        rec, f, lengths = self.significance_records(matrix, del_, ext, seed, per_pair, max_trim, w, pair_base, scores, **kw)
        out = significance_from_records(rec, self.f[w])
        return (out, f, lengths) if scores else out

    def p_values(self, matrix, del_, ext, seed, per_pair=statistics.SEQUENCES - 1, max_trim=6, keep=None, pair_base=0, slice_hits=64, **kw):
        """The reference's own p-value (calculate_p_value, statistics/mod.rs:240-307) of every listed hit: scores [f_hit] + the f of
        its copies, lengths [len(target)] + theirs, exactly as statistics.calculate_p_values composes them, through the same
        calculate_distribution_params / get_p_value (host numpy).  The copies' scores come down slice_hits hits at a time.  A failed
        copy raises, as the reference's unwrap panics."""
        o = self.owner
        w = self._keep(keep)
        out = np.empty(len(w), dtype=np.float64)
        for a in range(0, len(w), max(int(slice_hits), 1)):
            part = w[a:a + max(int(slice_hits), 1)]
            rec, f, lengths = self.significance_records(matrix, del_, ext, seed, per_pair, max_trim, part, pair_base, True, **kw)
            bad = rec["status"] != _ffi.OK
            if bad.any():
                runtime.raise_for_status(int(rec["status"][bad][0]), "aln_seqset_held_significance")
            for i, h in enumerate(part):
                ql, tl, fh = int(o.len[self.q[h]]), int(o.len[self.t[h]]), float(self.f[h])
                sc = np.concatenate([[fh], f[i]])
                ln = np.concatenate([[tl], lengths[i].astype(np.int64)])
                out[a + i] = float(statistics.calculate_distribution_params(ql, ln, sc).get_p_value(ql, tl, fh))
        return out

    def _report_params(self, matrix, blank):
        # (only matrix / rows / cols / row_stride / blank_code are read)
        return runtime.make_params(self.semantics, 0.0, 0.0, matrix, outputs=_ffi.OUT_SCORE, blank=blank)

    def report(self, matrix, keep=None, skip_seed=True, blank=98):
        """aln_seqset_held_report: the classed columns of the listed positions of the held list (default: all) as a REPORT_DTYPE
        array -- columns, identical, positive, mismatch, q_gap, t_gap, q_gap_open, t_gap_open, status -- counted on the device in the
        classes of Alignment.get_alignment(matrix).  skip_seed leaves out the last column, the traceback's seed pair, which repeats
        residues the walk emits itself; without it the counts are those of the reference's own midline."""
        o = self.owner
        w = self._keep(keep)
        p, _held = self._report_params(matrix, blank)
        rep = np.zeros(len(w), dtype=REPORT_DTYPE)
        st = o.lib.aln_seqset_held_report(o.handle, C.byref(p), _ffi.REPORT_SKIP_SEED if skip_seed else 0, w.ctypes.data, len(w), rep.ctypes.data)
        runtime.raise_for_status(st, "aln_seqset_held_report")
        return rep

    def filter(self, matrix, min_identity=0.0, min_q_cover=0.0, min_t_cover=0.0, min_columns=0, skip_seed=True, with_reports=False, blank=98,
               capacity=None):
        """aln_seqset_held_filter: the positions of the held hits with identical >= min_identity * columns, columns - q_gap >=
        min_q_cover * N, columns - t_gap >= min_t_cover * M and columns >= min_columns, ascending, selected on the device; only they
        come down.  with_reports: (positions, their REPORT_DTYPE records).  capacity (default: every held hit) bounds what is
        written; .last_filter_count is the number kept in all."""
        o = self.owner
        p, _held = self._report_params(matrix, blank)
        cap = self.count if capacity is None else int(capacity)
        flt = _ffi.HitFilter(float(min_identity), float(min_q_cover), float(min_t_cover), int(min_columns), 0)
        pos = np.zeros(cap, dtype=np.uint32)
        rep = np.zeros(cap, dtype=REPORT_DTYPE) if with_reports else None
        count = C.c_uint64(0)
        st = o.lib.aln_seqset_held_filter(o.handle, C.byref(p), _ffi.REPORT_SKIP_SEED if skip_seed else 0, C.byref(flt), pos.ctypes.data,
                                          rep.ctypes.data if with_reports else None, cap, C.byref(count))
        runtime.raise_for_status(st, "aln_seqset_held_filter")
        self.last_filter_count = int(count.value)
        n = min(self.last_filter_count, cap)
        return (pos[:n], rep[:n]) if with_reports else pos[:n]

    def cluster(self, matrix=None, mode="components", min_identity=0.0, min_q_cover=0.0, min_t_cover=0.0, min_columns=0, skip_seed=True, blank=98,
                capacity=None):
        """aln_seqset_held_cluster: the sequences of the held pass's block grouped by the held hits, on the device; 4 bytes per
        sequence and 16 per cluster come down.  mode "components": single linkage, label = the smallest member; "greedy":
        longest-first representatives, a sequence joins the first representative it has a kept hit with.  With a matrix the edges
        are the hits that filter(matrix, min_...) keeps; without one (and without thresholds) every held hit that succeeded.
        Returns a cluster.Clusters; sequences outside the block carry the label cluster.NONE."""
        from . import cluster as _cluster
        o = self.owner
        thresholds = bool(min_identity or min_q_cover or min_t_cover or min_columns)
        if matrix is None and thresholds:
            raise ValueError("aln_seqset_held_cluster: thresholds need the matrix their classes are counted under")
        n = len(o)
        cap = n if capacity is None else int(capacity)
        label = np.zeros(n, dtype=np.uint32)
        rec = np.zeros(cap, dtype=_cluster.RECORD_DTYPE)
        summ = _ffi.ClusterSummary()
        if matrix is None:
            p_ref, flt_ref, flags = None, None, 0
        else:
            p, _held = self._report_params(matrix, blank)
            flt = _ffi.HitFilter(float(min_identity), float(min_q_cover), float(min_t_cover), int(min_columns), 0)
            p_ref, flt_ref, flags = C.byref(p), C.byref(flt), _ffi.REPORT_SKIP_SEED if skip_seed else 0
        st = o.lib.aln_seqset_held_cluster(o.handle, p_ref, flags, flt_ref, _cluster.mode_code(mode), label.ctypes.data, rec.ctypes.data if cap else None,
                                           cap, C.byref(summ))
        runtime.raise_for_status(st, "aln_seqset_held_cluster")
        return _cluster.Clusters(label, rec[:min(int(summ.clusters), cap)], _cluster.summary_dict(summ))

    def profiles(self, labels, centers=None, n_codes=None, matrix=None, min_identity=0.0, min_q_cover=0.0, min_t_cover=0.0, min_columns=0,
                 skip_seed=True, blank=98):
        """aln_seqset_held_profiles: for every centre and every residue position of it, how often each residue code, a deletion or
        any other code of its family's members is aligned to it in the held hits -- counted on the device; one uint32 matrix per
        centre comes down.  labels: one per sequence (an array, or the Clusters of .cluster); a hit (q, t) counts iff both carry the
        same label and exactly one of them is that label, the centre.  centers (default: the labels that have at least one other
        member): ascending sequence numbers.  n_codes (default: alphabet.volume()): the codes with a row of their own.  With a
        matrix only the hits that filter(matrix, min_...) keeps count.  Returns a profile.Profiles."""
        from . import profile as _profile
        o = self.owner
        thresholds = bool(min_identity or min_q_cover or min_t_cover or min_columns)
        if matrix is None and thresholds:
            raise ValueError("aln_seqset_held_profiles: thresholds need the matrix their classes are counted under")
        label = _profile.labels_of(labels)
        if label.shape != (len(o),):
            raise ValueError("aln_seqset_held_profiles: one label per sequence of the set")
        cen = _profile.default_centers(label) if centers is None else np.ascontiguousarray(centers, dtype=np.uint32)
        codes = _profile.check_codes(o.alphabet.volume() if n_codes is None else n_codes)
        total = C.c_uint64(0)
        st = o.lib.aln_seqset_profile_elements(o.handle, cen.ctypes.data if len(cen) else None, len(cen), codes, C.byref(total))
        runtime.raise_for_status(st, "aln_seqset_profile_elements")
        out = np.zeros(int(total.value), dtype=np.uint32)
        rec = np.zeros(len(cen), dtype=_profile.RECORD_DTYPE)
        summ = _ffi.ProfileSummary()
        if matrix is None:
            p_ref, flt_ref = None, None
        else:
            p, _held = self._report_params(matrix, blank)
            flt = _ffi.HitFilter(float(min_identity), float(min_q_cover), float(min_t_cover), int(min_columns), 0)
            p_ref, flt_ref = C.byref(p), C.byref(flt)
        st = o.lib.aln_seqset_held_profiles(o.handle, p_ref, _ffi.PROFILE_SKIP_SEED if skip_seed else 0, flt_ref, label.ctypes.data if len(label) else None,
                                            cen.ctypes.data if len(cen) else None, len(cen), codes, out.ctypes.data if len(out) else None, len(out),
                                            rec.ctypes.data if len(cen) else None, C.byref(summ))
        runtime.raise_for_status(st, "aln_seqset_held_profiles")

        def own(i):
            a = int(o.off[cen[i]])
            return o.seqs[a:a + int(o.len[cen[i]])]

        return _profile.Profiles(cen, o.len, own, codes, out, rec, _profile.summary_dict(summ))

    def msa(self, labels, centers=None, matrix=None, min_identity=0.0, min_q_cover=0.0, min_t_cover=0.0, min_columns=0, blank=98):
        """aln_seqset_held_msa_plan + aln_seqset_held_msa_fill: for every centre one matrix of residue codes -- row 0 the centre, then
        one row per held hit between the centre and a member of its family, in ascending held position -- in one set of columns, the
        members' inserts included (centre-star), laid out and written on the device; only the matrices and row lists come down.
        labels, centers, matrix and the thresholds as .profiles takes them; the traceback's seed column is never part of it.  Returns
        an msa.FamilyAlignments."""
        from . import msa as _msa
        from . import profile as _profile
        o = self.owner
        thresholds = bool(min_identity or min_q_cover or min_t_cover or min_columns)
        if matrix is None and thresholds:
            raise ValueError("aln_seqset_held_msa_plan: thresholds need the matrix their classes are counted under")
        label = _profile.labels_of(labels)
        if label.shape != (len(o),):
            raise ValueError("aln_seqset_held_msa_plan: one label per sequence of the set")
        cen = _profile.default_centers(label) if centers is None else np.ascontiguousarray(centers, dtype=np.uint32)
        rec = np.zeros(len(cen), dtype=_msa.RECORD_DTYPE)
        summ = _ffi.MsaSummary()
        if matrix is None:
            p_ref, flt_ref = None, None
        else:
            p, _held = self._report_params(matrix, blank)
            flt = _ffi.HitFilter(float(min_identity), float(min_q_cover), float(min_t_cover), int(min_columns), 0)
            p_ref, flt_ref = C.byref(p), C.byref(flt)
        st = o.lib.aln_seqset_held_msa_plan(o.handle, p_ref, 0, flt_ref, label.ctypes.data if len(label) else None, cen.ctypes.data if len(cen) else None,
                                            len(cen), rec.ctypes.data if len(cen) else None, C.byref(summ))
        runtime.raise_for_status(st, "aln_seqset_held_msa_plan")
        self.last_msa_plan_stats = o.stats()
        out = np.zeros(int(summ.bytes), dtype=np.uint8)
        row_hit = np.zeros(int(summ.total_rows), dtype=np.uint32)
        st = o.lib.aln_seqset_held_msa_fill(o.handle, out.ctypes.data if len(out) else None, len(out), row_hit.ctypes.data if len(row_hit) else None,
                                            len(row_hit))
        runtime.raise_for_status(st, "aln_seqset_held_msa_fill")
        # (without a matrix the device used the held pass's blank code: the one the pass was given)
        return _msa.FamilyAlignments(cen, rec, _msa.summary_dict(summ), out, row_hit, self.q, self.t, o.alphabet, blank)

    def cigars(self, keep=None, extended=False, clips=False, stranded=False):
        """aln_seqset_held_cigar_plan + aln_seqset_held_cigar_fill: the alignments of the listed positions of the held list (default:
        all) as CIGARs, run-length encoded on the device from the held strings -- per hit a few 32-bit words in BAM's encoding and a
        32-byte record (coordinates, matches, block length); the strings stay where they are.  extended: `=` / `X` in place of `M`;
        clips: soft clips for the query's residues outside the alignment.  stranded (a SeqSet.stranded only):
        aln_seqset_held_strand_cigar_plan / _fill -- the coordinates on the original records, the words along the forward target, and
        .q_rec, .t_rec, .strand beside them.  Returns a cigar.Cigars."""
        from . import cigar as _cigar
        o = self.owner
        w = self._keep(keep)
        flags = (_ffi.CIGAR_EXTENDED if extended else 0) | (_ffi.CIGAR_CLIPS if clips else 0)
        rec = np.zeros(len(w), dtype=_cigar.RECORD_DTYPE)
        summ = _ffi.CigarSummary()
        strands = None
        if stranded:
            strands = np.zeros(len(w), dtype=_cigar.STRAND_DTYPE)
            st = o.lib.aln_seqset_held_strand_cigar_plan(o.handle, flags, w.ctypes.data if len(w) else None, len(w), rec.ctypes.data if len(w) else None,
                                                         strands.ctypes.data if len(w) else None, C.byref(summ))
            runtime.raise_for_status(st, "aln_seqset_held_strand_cigar_plan")
        else:
            st = o.lib.aln_seqset_held_cigar_plan(o.handle, flags, w.ctypes.data if len(w) else None, len(w), rec.ctypes.data if len(w) else None,
                                                  C.byref(summ))
            runtime.raise_for_status(st, "aln_seqset_held_cigar_plan")
        self.last_cigar_plan_stats = o.stats()
        words = np.zeros(int(summ.total_ops), dtype=np.uint32)
        offsets = np.zeros(len(w) + 1, dtype=np.uint64)
        fill = o.lib.aln_seqset_held_strand_cigar_fill if stranded else o.lib.aln_seqset_held_cigar_fill
        st = fill(o.handle, words.ctypes.data if len(words) else None, len(words), offsets.ctypes.data, len(offsets))
        runtime.raise_for_status(st, "aln_seqset_held_strand_cigar_fill" if stranded else "aln_seqset_held_cigar_fill")
        return _cigar.Cigars(w, rec, _cigar.summary_dict(summ), offsets, words, flags, strands)

    def fractions(self, reports, keep=None):
        """report_fractions of records that belong to the listed positions (default: all)."""
        w = self._keep(keep)
        return report_fractions(reports, self.owner.len[self.q[w]], self.owner.len[self.t[w]])

    def alignments(self, keep=None):
        """Alignment objects of the listed positions (default: all), coordinates as SimpleLocalAligner / SimpleGlobalAligner give them."""
        o = self.owner
        w = np.arange(self.count, dtype=np.uint32) if keep is None else np.ascontiguousarray(keep, dtype=np.uint32)
        res, strs = self.strings(w)
        out = []
        for k in range(len(w)):
            r = res[k]
            runtime.raise_for_status(int(r["status"]), "aln_seqset_held_strings")
            if self.semantics == _ffi.CORE_GLOBAL:
                coords = ((1, int(o.len[self.q[w[k]]])), (1, int(o.len[self.t[w[k]]])))
            else:
                coords = ((int(r["start_x"]) + 1, int(r["end_x"]) + 1), (int(r["start_y"]) + 1, int(r["end_y"]) + 1))
            out.append(Alignment(o.alphabet, strs[k][0], strs[k][1], coords, float(r["f"])))
        return out


def best_ranks(q, t, f):
    """Rank of every entry within its query under the rule of aln_best_rules.h: higher f first, equal f (-0.0 == +0.0) by the lower
    target number."""
    q, t, f = np.asarray(q), np.asarray(t), np.asarray(f, dtype=np.float64)
    order = np.lexsort((t, -f, q))
    rank = np.zeros(len(q), dtype=np.uint32)
    if len(q):
        qs = q[order]
        start = np.flatnonzero(np.concatenate([[True], qs[1:] != qs[:-1]]))
        first = np.repeat(start, np.diff(np.concatenate([start, [len(q)]])))
        rank[order] = (np.arange(len(q)) - first).astype(np.uint32)
    return rank


class BestHits(HeldHits):
    """The held list of SeqSet.best: ascending pair order (query by query, targets ascending) as HeldHits, plus .rank -- 0 for a
    query's best target -- computed here from f and t by the rule.  by_query() yields (q, positions in rank order)."""

    def __init__(self, owner, count, semantics):
        super().__init__(owner, count, semantics)
        self.rank = best_ranks(self.q, self.t, self.f)

    def by_query(self):
        order = np.lexsort((self.rank, self.q))
        qs = self.q[order]
        cuts = np.flatnonzero(qs[1:] != qs[:-1]) + 1 if len(qs) else np.zeros(0, dtype=np.int64)
        for part in np.split(order, cuts):
            if len(part):
                yield int(self.q[part[0]]), part


def all_pairs(records, matrix, del_, ext, f_min=None, alphabet=Protein, semantics=_ffi.CORE_LOCAL, device=None, prefilter=None, **kw):
    """Every pair i < j of `records` (code arrays or strings) in generate_pairs order.  Without f_min: (q, t, f, status) arrays over
    all pairs.  With f_min: (q, t, f, alignments) of the pairs with f >= f_min.  prefilter=dict(k=, alphabet_size=[, min_shared=,
    min_per_1024=]): only the candidates of SeqSet.prefilter are aligned, and the arrays run over them."""
    with SeqSet(records, alphabet, device=device) as ss:
        n = len(ss)
        if prefilter is not None:
            cand = ss.prefilter(block=None, **prefilter)
            if f_min is None:
                f, status = cand.score(matrix, del_, ext, semantics=semantics, **kw)
                return cand.q, cand.t, f, status
            held = cand.hits(matrix, del_, ext, f_min, semantics=semantics, **kw)
            return held.q, held.t, held.f, held.alignments()
        if f_min is None:
            f, status = ss.score(matrix, del_, ext, None, semantics=semantics, **kw)
            q, t = np.triu_indices(n, 1)
            return q.astype(np.uint32), t.astype(np.uint32), f, status
        held = ss.hits(matrix, del_, ext, f_min, None, semantics=semantics, **kw)
        return held.q, held.t, held.f, held.alignments()
