"""python -m aligner_amd.allpairs -i x.fasta [--f-min F]: every pair i < j of a FASTA, scored on the device.

The request path of the reference (aligner-web dispatcher: generate_pairs, handlers.rs:253-264) as a command: prints
`q_head,t_head,f` per pair in generate_pairs order -- all pairs, or with --f-min only those with f >= F.  Local alignment, BLOSUM62,
gap opening 11, extension 2 unless told otherwise.

With --heuristic every pair runs the loop of HeuristicAligner instead (heuristic.align_set: local alignment under a matrix re-estimated
from the pair's own alignment until f stops growing), --kd K and --r-squared R being its parameters and --frequencies a,b,... the
residue frequencies (default: those of the FASTA over the alphabet's volume); a pair the reference panics on prints the panic.

With --best K the question is a database search's: per record, its K best partners among all the others (higher f first, equal f by
the earlier record), optionally only those with f >= F, selected on the device; prints `q_head,rank,t_head,f`, records in input
order, ranks from 1.  Not with --heuristic.

With --shuffles N (and --best or --f-min: a held pass) every printed hit is also asked whether it is better than chance: its query
against N trimmed and shuffled copies of its target, drawn, scored and reduced on the device; `,z,p_emp` is appended to each row
(z = (f - mean) / sd over the copies, p_emp = (copies with f >= the hit's + 1) / (copies + 1)).  --seed S picks the copies (default
0: the same output every run).  A hit whose target has fewer than 6 residues has no such copies (each loses up to 6 tail residues): its
row ends in `,nan,nan`.  Not with --heuristic.

With --report (and --best or --f-min) every printed hit also says how identical, how covering and how gapped its alignment is:
`,columns,identity,positives,q_cover,t_cover,gap_opens,gaps` is appended to each row (after `,z,p_emp` with --shuffles), counted on
the device over the alignment's columns (the traceback's duplicated seed column left out): identity = identical / columns, positives
= (identical + positive-scoring) / columns, q_cover / t_cover = aligned residues of the first / second record over its length.
--min-identity X, --min-q-cover Y, --min-t-cover Z print only the hits the device filter keeps (with --best the K best are selected
first, then filtered); --shuffles then runs on the kept hits only.  Not with --heuristic.

With --cluster components|greedy (and --best or --f-min) the records are grouped by the held hits on the device and the hit rows are
replaced by one row per record, in input order: `head,rep_head,cluster_size`.  components: single linkage, rep_head the first record
of the family; greedy: longest-first representatives, a record joins the first representative it has a hit with.  The --min-*
thresholds, when given, decide which hits count as edges.  Not with --heuristic, --shuffles or --report.

With --cluster ... --profiles FILE the profile of every family of two or more records is written to FILE as well, counted on the device
over the same hits: a header line `>rep_head hits=N` (N: the hits between the representative and a member of its family), then one
line per residue position of the representative with the comma-separated counts of the members' aligned codes -- one per code of the
alphabet, then deletions, then every other code (the traceback's duplicated seed column left out).  A hit between two members of a
family counts for no profile.

With --cluster ... --msa FILE the alignment of every family of two or more records is written to FILE as aligned FASTA, merged on the
device from the same hits (centre-star: every member as it is aligned to the representative, the members' inserts in columns of their
own): one block per family -- `>rep_head` and the representative's row, then `>member_head hit=H` and the row of every hit between
the representative and a member (H: the hit's position among the held hits) -- and a blank line; `-` where a row has no residue.

With --paf FILE (and --best, --best-candidates or --f-min: a held pass) every printed hit is also written to FILE as one PAF line, its
alignment run-length encoded on the device from the held strings: the 12 standard columns -- q_head, its length, start and end (0-based,
end exclusive), strand `+`, t_head, its length, start and end, the matching residues, the alignment's columns (the traceback's
duplicated seed column left out), mapping quality 255 -- then `af:f:<f>` and `cg:Z:<cigar>`; --eqx writes `=` / `X` in place of `M`.
The lines follow the rows' order; with --min-* only the kept hits are written.  Not with --heuristic or --cluster.

With --kmer K the pairs are prefiltered on the device first: only the candidates -- pairs whose records share at least --min-shared N
distinct words of K residues (default 0) and at least P / 1024 of the smaller record's distinct words (--min-shared-per-1024 P,
default 0) -- are aligned at all.  Words are counted over the first A codes of the alphabet (--kmer-alphabet A; default 20, the
standard residues, or 4 with --dna); a window that touches any other code is no word; A^K may not exceed 2^18.  With --f-min F the rows
and everything downstream (--report, --min-*, --shuffles, --cluster) are those of the candidates with f >= F; without it one row per
candidate is printed: `q_head,t_head,f,shared`.  The surviving alignments are bit for bit those of the unfiltered run; which pairs
survive is the thresholds' business.  Not with --best (which aligns every pair; see --best-candidates) or --heuristic.

With --kmer K --best-candidates N the question of --best is asked of the candidates only: per record, its N best partners among the
records it shares enough words with, optionally only those with f >= F (--f-min is the floor, as with --best), selected on the
device; prints --best's rows, `q_head,rank,t_head,f`, and takes --report, --min-*, --shuffles and --cluster on top.  The prefilter
runs on the full square of the records, which lists (q, t), (t, q) and every record's pair with itself: the self pairs are aligned
and then skipped.  Not with --best or --heuristic.

With --kmer K --word-join the same candidates come from a sorted word index instead of the bitmaps: every (word, record) is sorted once
and the records that carry a word name the pairs that share it, so the work follows what is shared and A^K may be as large as 2^32
(proteins: K up to 7).  --min-shared defaults to 1 here and may not be 0: a join sees only pairs that share a word.  Everything that
combines with --kmer combines with --kmer --word-join; where both routes apply they print the same rows.

With --kmer K --seed-join the candidates come from word hits that lie on a common diagonal: every occurrence of a word keeps its
position, a seed is a word at position pq of the first record and pt of the second, its diagonal pt - pq, and a pair is a candidate
if some band of diagonals d0 .. d0 + B (--band B, default 0) holds at least --min-seeds N seeds (default 1).  Words with more than
--max-occ C occurrences in the whole set make no seed (default 0: none is dropped).  K goes up to 16 on this route (A^K up to 2^32).
Not with --word-join, --min-shared or --min-shared-per-1024.  Rows without --f-min are `q_head,t_head,f,seeds,diag`: the seeds of the
best band and its least diagonal.  Everything that combines with --kmer --word-join combines with --kmer --seed-join, --both-strands
and --best-candidates included; against a reverse-complement partner the diagonal is in the mirror's coordinates (position p of the
mirror is position length - 1 - p of the record).

With --kmer K --seed-join --chain (or --word-join --chain) the candidates are filtered, before any pass, by the colinear chain over ALL
their seeds (anchors: every (pq, pt) with the same, not dropped, word at both), chained on the device from the seed index alone: an
anchor may follow another that lies before it on both records, within --max-gap G on either (default 1000) and within --max-skew B of
diagonal drift (default 200); a link gains min(the two distances, K) and costs drift / 8; a chain's score is K plus its links'.  A
candidate is kept if its best chain scores at least --min-chain-score S (default 0) and spans at least --min-chain-span L residues on
both records (default 0), or if it has more than 2^16 anchors and is not chained at all (never lost for being expensive; its chain
columns are 0).  Rows without --f-min gain `chain_score,anchors,q_start,q_end,t_start,t_end` (after `diag` with --seed-join): the
chain's score, its anchors, and where it starts and ends (0-based, end exclusive) on the two records; against a reverse-complement
partner the target positions are in the mirror's coordinates, as diag is.  --chain-paf FILE writes one approximate PAF line per printed
candidate WITHOUT any fill: the 12 columns with residue matches = anchors * K capped at the shorter span and block length = the longer
span, mapping quality 255, then `cs:i:<score>` and `cn:i:<anchors>`, no `cg`; with --both-strands strand `-` and the coordinates on the
original records, converted as --paf converts them.  Every option that combines with --seed-join combines with --chain unchanged.

With --dna --both-strands every record is also held as its reverse complement, made on the device behind the records, and every pass is
one rectangle: each record as the query against every record on both strands.  Every row gains a `strand` column after t_head -- `+`, or
`-` where the partner matches as its reverse complement; t_head is the original record's header.  A pair (i, j) is computed from both
sides; the rows of all pairs, of --f-min and of --kmer print it once per strand, from the record that comes first in the file (a block
shape for "i < j across strands" is not built), so a record against its own reverse complement is not among them; --best and
--best-candidates print per record as always, a record's own reverse complement included, and may name a partner on both strands.
--paf writes the strand, the coordinates on the original records and the CIGAR along the forward target.  --report, --min-* and
--shuffles work unchanged.  --cluster, --profiles, --msa and --heuristic over both strands are not built.
"""
import argparse
import sys

import numpy as np

from . import _ffi
from .enums import DNA, Protein
from .fasta import encode_records, read_fasta
from .matrices import get_blosum62, nucleotide_matrix
from .seqset import SeqSet, both, rectangle


MAX_TRIM = 6          # tail residues a shuffled copy may lose (statistics/mod.rs:312-314)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m aligner_amd.allpairs", description=__doc__.split("\n\n")[0])
    ap.add_argument("-i", "--input", required=True, help="FASTA with two or more records")
    ap.add_argument("--f-min", type=float, default=None, help="print only the pairs with f >= F")
    ap.add_argument("--del", dest="del_", type=float, default=11.0)
    ap.add_argument("--ext", type=float, default=2.0)
    ap.add_argument("--global", dest="global_", action="store_true", help="global instead of local alignment")
    ap.add_argument("--dna", action="store_true", help="nucleotide records (match 5, mismatch -4)")
    ap.add_argument("--device", type=int, default=None)
    ap.add_argument("--heuristic", action="store_true", help="the matrix re-estimation loop per pair (needs --kd and --r-squared)")
    ap.add_argument("--kd", type=float, default=None)
    ap.add_argument("--r-squared", type=float, default=None)
    ap.add_argument("--frequencies", default=None, help="comma-separated residue frequencies, one per code of the alphabet")
    ap.add_argument("--best", type=int, default=None, metavar="K", help="per record its K best partners (1 .. %d), self pairs skipped" % _ffi.SEQSET_BEST_MAX)
    ap.add_argument("--shuffles", type=int, default=None, metavar="N", help="append z,p_emp from N shuffled copies of each hit's target (with --best or --f-min)")
    ap.add_argument("--seed", type=int, default=None, help="seed of the shuffled copies (default 0)")
    ap.add_argument("--report", action="store_true", help="append columns,identity,positives,q_cover,t_cover,gap_opens,gaps (with --best or --f-min)")
    ap.add_argument("--min-identity", type=float, default=None, metavar="X", help="print only hits with identical >= X * columns (with --best: the K best are selected first, then filtered)")
    ap.add_argument("--min-q-cover", type=float, default=None, metavar="Y", help="print only hits whose alignment covers Y of the first record (with --best: selected first, then filtered)")
    ap.add_argument("--min-t-cover", type=float, default=None, metavar="Z", help="print only hits whose alignment covers Z of the second record (with --best: selected first, then filtered)")
    ap.add_argument("--cluster", choices=("components", "greedy"), default=None, help="group the records by the held hits: prints head,rep_head,cluster_size per record (with --best or --f-min)")
    ap.add_argument("--profiles", default=None, metavar="FILE", help="with --cluster: write every family's per-position residue counts to FILE")
    ap.add_argument("--msa", default=None, metavar="FILE", help="with --cluster: write every family's alignment to FILE as aligned FASTA")
    ap.add_argument("--paf", default=None, metavar="FILE", help="write every printed hit to FILE as a PAF line with its CIGAR (with --best, --best-candidates or --f-min)")
    ap.add_argument("--eqx", action="store_true", help="with --paf: = and X in place of M")
    ap.add_argument("--kmer", type=int, default=None, metavar="K", help="prefilter: align only the pairs that share enough words of K residues (1 .. %d)" % _ffi.PREFILTER_MAX_K)
    ap.add_argument("--min-shared", type=int, default=None, metavar="N", help="with --kmer: candidates share at least N distinct words")
    ap.add_argument("--min-shared-per-1024", type=int, default=None, metavar="P", help="with --kmer: candidates share at least P / 1024 of the smaller record's distinct words (0 .. 1024)")
    ap.add_argument("--kmer-alphabet", type=int, default=None, metavar="A", help="with --kmer: words use the first A codes of the alphabet (default 20; 4 with --dna)")
    ap.add_argument("--best-candidates", type=int, default=None, metavar="N",
                    help="with --kmer: per record its N best partners (1 .. %d) among its candidates on the full square; self pairs are aligned, then skipped" % _ffi.SEQSET_BEST_MAX)
    ap.add_argument("--word-join", action="store_true", help="with --kmer: the candidates by a join over a sorted word index; A^K up to 2^32, --min-shared at least 1 (default 1)")
    ap.add_argument("--seed-join", action="store_true",
                    help="with --kmer: the candidates by word hits on a common diagonal; K up to %d, A^K up to 2^32; rows gain seeds,diag (on a reverse-complement partner diag is in the mirror's coordinates)" % _ffi.SEEDJOIN_MAX_K)
    ap.add_argument("--min-seeds", type=int, default=None, metavar="N", help="with --seed-join: candidates have at least N seeds within one band of diagonals (default 1)")
    ap.add_argument("--band", type=int, default=None, metavar="B", help="with --seed-join: a band holds the diagonals d0 .. d0 + B (default 0)")
    ap.add_argument("--max-occ", type=int, default=None, metavar="C", help="with --seed-join: words with more than C occurrences in the whole set make no seed (default 0: none is dropped)")
    ap.add_argument("--chain", action="store_true", help="with --seed-join or --word-join: keep the candidates by the colinear chain over their seeds; rows gain chain_score,anchors,q_start,q_end,t_start,t_end")
    ap.add_argument("--max-gap", type=int, default=None, metavar="G", help="with --chain: chained seeds lie within G residues of each other on either record (default 1000)")
    ap.add_argument("--max-skew", type=int, default=None, metavar="B", help="with --chain: chained seeds drift at most B diagonals apart (default 200)")
    ap.add_argument("--min-chain-score", type=int, default=None, metavar="S", help="with --chain: keep the candidates whose chain scores at least S (default 0)")
    ap.add_argument("--min-chain-span", type=int, default=None, metavar="L", help="with --chain: keep the candidates whose chain spans at least L residues on both records (default 0)")
    ap.add_argument("--chain-paf", default=None, metavar="FILE", help="with --chain: write one approximate PAF line per printed candidate to FILE, without any fill")
    ap.add_argument("--both-strands", action="store_true", help="with --dna: also match every record as its reverse complement; rows gain a strand column")
    a = ap.parse_args(argv)
    if a.both_strands:
        if not a.dna:
            ap.error("--both-strands is the reverse complement of nucleotide records: give --dna")
        for given, name in ((a.cluster is not None, "--cluster"), (a.profiles is not None, "--profiles"), (a.msa is not None, "--msa"), (a.heuristic, "--heuristic")):
            if given:
                ap.error("--both-strands with %s is not built" % name)
    if a.word_join and a.kmer is None:
        ap.error("--word-join is a route of the prefilter: give --kmer K")
    if a.seed_join:
        if a.kmer is None:
            ap.error("--seed-join is a route of the prefilter: give --kmer K")
        if a.word_join:
            ap.error("--seed-join with --word-join: both name the route to the candidates; give one")
        if a.min_shared is not None or a.min_shared_per_1024 is not None:
            ap.error("--min-shared / --min-shared-per-1024 count distinct shared words: --seed-join counts seeds, its thresholds are --min-seeds, --band and --max-occ")
    elif a.min_seeds is not None or a.band is not None or a.max_occ is not None:
        ap.error("--min-seeds / --band / --max-occ are the thresholds of --seed-join: give --kmer K --seed-join")
    if a.chain_paf is not None and not a.chain:
        ap.error("--chain-paf writes the chains of --chain: give --chain")
    if a.chain:
        if a.kmer is None or not (a.seed_join or a.word_join):
            ap.error("--chain chains the seeds of a join's candidates: give --kmer K with --seed-join or --word-join")
    elif a.max_gap is not None or a.max_skew is not None or a.min_chain_score is not None or a.min_chain_span is not None:
        ap.error("--max-gap / --max-skew / --min-chain-score / --min-chain-span are the parameters of --chain: give --chain")
    if a.best_candidates is not None:
        if a.kmer is None:
            ap.error("--best-candidates selects among the prefilter's candidates: give --kmer K")
        if a.best is not None:
            ap.error("--best-candidates with --best: --best aligns every pair, --best-candidates only the candidates of --kmer; give one")
        if a.heuristic:
            ap.error("--best-candidates selects by the score of the plain alignment: not with --heuristic")
        if not 1 <= a.best_candidates <= _ffi.SEQSET_BEST_MAX:
            ap.error("--best-candidates: N must lie in 1 .. %d" % _ffi.SEQSET_BEST_MAX)
    if a.kmer is None:
        if a.min_shared is not None or a.min_shared_per_1024 is not None or a.kmer_alphabet is not None:
            ap.error("--min-shared / --min-shared-per-1024 / --kmer-alphabet are the prefilter's thresholds: give --kmer K")
    else:
        if a.best is not None:
            ap.error("--kmer with --best: --best aligns every pair; the per-record selection among the candidates is --best-candidates N")
        if a.heuristic:
            ap.error("--kmer with --heuristic: the matrix loop over a sparse candidate list is not built")
        kmer_alphabet = a.kmer_alphabet if a.kmer_alphabet is not None else (4 if a.dna else 20)
        if a.seed_join:
            if not 1 <= a.kmer <= _ffi.SEEDJOIN_MAX_K or kmer_alphabet < 1 or kmer_alphabet ** a.kmer > _ffi.SEEDJOIN_MAX_WORDS:
                ap.error("--kmer with --seed-join: K must lie in 1 .. %d and A^K may not exceed 2^32" % _ffi.SEEDJOIN_MAX_K)
            if a.min_seeds is not None and not 1 <= a.min_seeds < 2 ** 32:
                ap.error("--min-seeds: N must lie in 1 .. 2^32 - 1, a join sees only pairs that have a seed")
            if a.band is not None and not 0 <= a.band <= _ffi.SEEDJOIN_MAX_BAND:
                ap.error("--band: B must lie in 0 .. 2^31 - 1")
            if a.max_occ is not None and not 0 <= a.max_occ < 2 ** 32:
                ap.error("--max-occ: C must lie in 0 .. 2^32 - 1")
        elif a.word_join:
            if not 1 <= a.kmer <= _ffi.WORDJOIN_MAX_K or kmer_alphabet < 1 or kmer_alphabet ** a.kmer > _ffi.WORDJOIN_MAX_WORDS:
                ap.error("--kmer with --word-join: K must lie in 1 .. %d and A^K may not exceed 2^32" % _ffi.WORDJOIN_MAX_K)
            if a.min_shared is not None and a.min_shared < 1:
                ap.error("--min-shared with --word-join: N must be at least 1, a join sees only pairs that share a word")
        elif not 1 <= a.kmer <= _ffi.PREFILTER_MAX_K or kmer_alphabet < 1 or kmer_alphabet ** a.kmer > _ffi.PREFILTER_MAX_BITS:
            ap.error("--kmer: K must lie in 1 .. %d and A^K may not exceed 2^18" % _ffi.PREFILTER_MAX_K)
        if a.chain:
            if a.max_gap is not None and not 1 <= a.max_gap <= _ffi.SEEDCHAIN_MAX_GAP:
                ap.error("--max-gap: G must lie in 1 .. 2^31 - 1")
            if a.max_skew is not None and not 0 <= a.max_skew <= _ffi.SEEDCHAIN_MAX_SKEW:
                ap.error("--max-skew: B must lie in 0 .. 2^31 - 1")
            if a.min_chain_score is not None and not -(2 ** 31) <= a.min_chain_score < 2 ** 31:
                ap.error("--min-chain-score: S must fit 32 signed bits")
            if a.min_chain_span is not None and not 0 <= a.min_chain_span < 2 ** 32:
                ap.error("--min-chain-span: L must lie in 0 .. 2^32 - 1")
        if a.min_shared is not None and not 0 <= a.min_shared < 2 ** 32:
            ap.error("--min-shared: N must lie in 0 .. 2^32 - 1")
        if a.min_shared_per_1024 is not None and not 0 <= a.min_shared_per_1024 <= 1024:
            ap.error("--min-shared-per-1024: P must lie in 0 .. 1024")
    filtered = a.min_identity is not None or a.min_q_cover is not None or a.min_t_cover is not None
    if a.report or filtered:
        if a.heuristic:
            ap.error("--report / --min-identity / --min-q-cover / --min-t-cover describe the plain alignment: not with --heuristic")
        if a.best is None and a.best_candidates is None and a.f_min is None:
            ap.error("--report / --min-identity / --min-q-cover / --min-t-cover work on held hits: give --best K, --best-candidates N or --f-min F")
    if a.eqx and a.paf is None:
        ap.error("--eqx chooses the ops of --paf: give --paf FILE")
    if a.paf is not None:
        if a.heuristic:
            ap.error("--paf writes the plain alignment's hits: not with --heuristic")
        if a.cluster is not None:
            ap.error("--paf writes the hit rows, which --cluster replaces: not with --cluster")
        if a.best is None and a.best_candidates is None and a.f_min is None:
            ap.error("--paf works on held hits: give --best K, --best-candidates N or --f-min F")
    if a.profiles is not None and a.cluster is None:
        ap.error("--profiles counts the families of --cluster: give --cluster components|greedy")
    if a.msa is not None and a.cluster is None:
        ap.error("--msa aligns the families of --cluster: give --cluster components|greedy")
    if a.cluster is not None:
        if a.heuristic:
            ap.error("--cluster groups by the plain alignment's hits: not with --heuristic")
        if a.best is None and a.best_candidates is None and a.f_min is None:
            ap.error("--cluster works on held hits: give --best K, --best-candidates N or --f-min F")
        if a.shuffles is not None or a.report:
            ap.error("--cluster replaces the hit rows: not with --shuffles or --report")
    if a.shuffles is not None:
        if a.heuristic:
            ap.error("--shuffles asks about the plain alignment's score: not with --heuristic")
        if a.best is None and a.best_candidates is None and a.f_min is None:
            ap.error("--shuffles works on held hits: give --best K, --best-candidates N or --f-min F")
        if not 1 <= a.shuffles <= _ffi.SHUFFLE_MAX_COPIES:
            ap.error("--shuffles: N must lie in 1 .. %d" % _ffi.SHUFFLE_MAX_COPIES)
    elif a.seed is not None:
        ap.error("--seed picks the copies of --shuffles")
    records = read_fasta(a.input)
    if len(records) < 2:
        ap.error("%s: an all-against-all run needs two or more records" % a.input)
    alphabet = DNA if a.dna else Protein
    matrix = nucleotide_matrix() if a.dna else get_blosum62()
    sem = _ffi.CORE_GLOBAL if a.global_ else _ffi.CORE_LOCAL
    heads = [r.head.decode("utf-8", "replace") for r in records]
    out = sys.stdout
    n_rec = len(records)

    def make_set(codes):
        return SeqSet.stranded(codes, alphabet, device=a.device) if a.both_strands else SeqSet(codes, alphabet, device=a.device)

    def square(ss):
        """every record as the query against every resident record: with --both-strands the mirrors too"""
        return both(rectangle(0, n_rec, 0, n_rec), n_rec) if a.both_strands else rectangle(0, len(ss), 0, len(ss))

    def t_cols(t):
        """the row's t_head, and with --both-strands the strand column behind it"""
        t = int(t)
        return "%s,%s" % (heads[t % n_rec], "-" if t >= n_rec else "+") if a.both_strands else heads[t]

    def once(q, t):
        """--both-strands, rows that are not per record: which of the rectangle's pairs are printed -- each pair and strand from the
        record that comes first"""
        return np.asarray(q, dtype=np.int64) < np.asarray(t, dtype=np.int64) % n_rec

    def kept(held):
        """positions of the held list that are printed (None: all) and their reports (None without --report)"""
        if filtered:
            got = held.filter(matrix, min_identity=a.min_identity or 0.0, min_q_cover=a.min_q_cover or 0.0, min_t_cover=a.min_t_cover or 0.0,
                              with_reports=a.report)
            return got if a.report else (got, None)
        return None, (held.report(matrix) if a.report else None)

    def clustered(held):
        """--cluster: one row per record that is a node, in record order"""
        got = held.cluster(matrix if filtered else None, mode=a.cluster, min_identity=a.min_identity or 0.0, min_q_cover=a.min_q_cover or 0.0,
                           min_t_cover=a.min_t_cover or 0.0)
        size = dict(zip(got.records["label"].tolist(), got.records["size"].tolist()))
        for i, lab in enumerate(got.label.tolist()):
            if lab != _ffi.CLUSTER_NONE:
                out.write("%s,%s,%d\n" % (heads[i], heads[lab], size[lab]))
        if a.profiles is not None:
            prof = held.profiles(got, matrix=matrix if filtered else None, min_identity=a.min_identity or 0.0, min_q_cover=a.min_q_cover or 0.0,
                                 min_t_cover=a.min_t_cover or 0.0)
            with open(a.profiles, "w") as fh:
                for i, r in enumerate(prof.records):
                    fh.write(">%s hits=%d\n" % (heads[int(r["center"])], int(r["hits"])))
                    for column in prof.counts(i).T.tolist():
                        fh.write(",".join(str(x) for x in column) + "\n")
        if a.msa is not None:
            fam = held.msa(got, matrix=matrix if filtered else None, min_identity=a.min_identity or 0.0, min_q_cover=a.min_q_cover or 0.0,
                           min_t_cover=a.min_t_cover or 0.0)
            with open(a.msa, "w") as fh:
                for i in range(len(fam)):
                    names = [">%s" % heads[int(fam.centers[i])]] + [">%s hit=%d" % (heads[int(m)], int(h)) for m, h in zip(fam.members(i)[1:], fam.hits(i))]
                    for name, row in zip(names, fam.text(i)):
                        fh.write("%s\n%s\n" % (name, row))
                    fh.write("\n")

    def write_paf(held, order):
        """--paf: one line per printed hit, `order` their held positions in the rows' order"""
        order = np.asarray(order, dtype=np.uint32)
        got = held.cigars(keep=order, extended=a.eqx, stranded=a.both_strands)
        length = held.owner.len
        with open(a.paf, "w") as fh:
            for i, h in enumerate(order.tolist()):
                q, t = (int(got.q_rec[i]), int(got.t_rec[i])) if a.both_strands else (int(held.q[h]), int(held.t[h]))
                fh.write(got.paf(i, heads[q], length[q], heads[t], length[t], held.f[h]) + "\n")

    def tail(held, pos=None, reports=None):
        """`,z,p_emp` and the report's columns per held position, or empty strings without --shuffles and --report; pos: the
        positions that are printed (None: all)"""
        rows = [""] * len(held)
        shown = np.arange(len(held), dtype=np.uint32) if pos is None else np.asarray(pos, dtype=np.uint32)
        if a.shuffles is not None:
            # a copy loses up to MAX_TRIM tail residues: a target shorter than that has no such copies (the library refuses it)
            can = shown[held.owner.len[held.t[shown]] >= MAX_TRIM].astype(np.uint32)
            sig = held.significance(matrix, a.del_, a.ext, a.seed or 0, per_pair=a.shuffles, max_trim=MAX_TRIM, keep=can)
            for h in shown:
                rows[int(h)] = ",nan,nan"
            for h, z, p in zip(can, sig["z"], sig["p_emp"]):
                rows[int(h)] = ",%r,%r" % (float(z), float(p))
        if reports is not None:
            fr = held.fractions(reports, shown)
            for h, r, x in zip(shown, reports, fr):
                rows[int(h)] += ",%d,%r,%r,%r,%r,%d,%d" % (int(r["columns"]), float(x["identity"]), float(x["positives"]), float(x["q_cover"]),
                                                            float(x["t_cover"]), int(x["gap_opens"]), int(x["gaps"]))
        return rows

    def chain_paf(cand):
        """--chain-paf: one approximate line per printed candidate, from its chain record alone"""
        length = cand.owner.len
        shown = np.flatnonzero(once(cand.q, cand.t)) if a.both_strands else range(len(cand))
        with open(a.chain_paf, "w") as fh:
            for c in shown:
                r, q, t = cand.chain[c], int(cand.q[c]), int(cand.t[c])
                minus = a.both_strands and t >= n_rec
                t_len, ts, te = int(length[t]), int(r["t_start"]), int(r["t_end"])
                if minus:
                    ts, te = t_len - te, t_len - ts
                sq, st = int(r["q_end"]) - int(r["q_start"]), te - ts
                fh.write("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tcs:i:%d\tcn:i:%d\n" % (
                    heads[q], int(length[q]), int(r["q_start"]), int(r["q_end"]), "-" if minus else "+", heads[t % n_rec], t_len, ts, te,
                    min(int(r["anchors"]) * a.kmer, sq, st), max(sq, st), int(r["score"]), int(r["anchors"])))

    def candidates(ss, block):
        """the candidate list of --kmer over the block, by the bitmaps or, with --word-join, by the sorted word index or, with
        --seed-join, by the seeds on a common diagonal; with --chain, filtered by the chain over their seeds"""
        if not a.chain:
            return joined(ss, block)
        if not a.seed_join:
            ss.seed_index(a.kmer, kmer_alphabet)       # before the list is made: a new index drops it
        cand = joined(ss, block).chain_filter(a.min_chain_score or 0, a.min_chain_span or 0, max_gap=1000 if a.max_gap is None else a.max_gap,
                                              max_skew=200 if a.max_skew is None else a.max_skew, max_occ=a.max_occ or 0, k=a.kmer,
                                              alphabet_size=kmer_alphabet)
        if a.chain_paf is not None:
            chain_paf(cand)
        return cand

    def joined(ss, block):
        if a.seed_join:
            return ss.seed_join(a.kmer, kmer_alphabet, min_seeds=1 if a.min_seeds is None else a.min_seeds, band=a.band or 0, max_occ=a.max_occ or 0,
                                block=block)
        if a.word_join:
            return ss.word_join(a.kmer, kmer_alphabet, min_shared=1 if a.min_shared is None else a.min_shared,
                                min_per_1024=a.min_shared_per_1024 or 0, block=block)
        return ss.prefilter(a.kmer, kmer_alphabet, min_shared=a.min_shared or 0, min_per_1024=a.min_shared_per_1024 or 0, block=block)

    if a.best is not None or a.best_candidates is not None:
        if a.heuristic:
            ap.error("--best selects by the score of the plain alignment: not with --heuristic")
        if a.best is not None and not 1 <= a.best <= _ffi.SEQSET_BEST_MAX:
            ap.error("--best: K must lie in 1 .. %d" % _ffi.SEQSET_BEST_MAX)
        floor = float("-inf") if a.f_min is None else a.f_min
        with make_set(encode_records(records, alphabet)) as ss:
            if a.best is not None:
                held = ss.best(matrix, a.del_, a.ext, a.best, f_min=floor, block=square(ss), skip_self=True, semantics=sem)
            else:
                cand = candidates(ss, square(ss))
                held = cand.best(matrix, a.del_, a.ext, a.best_candidates, f_min=floor, skip_self=True, semantics=sem)
            if a.cluster is not None:
                clustered(held)
                return 0
            pos_kept, reports = kept(held)
            more = tail(held, pos_kept, reports)
            show = np.ones(len(held), dtype=bool) if pos_kept is None else np.isin(np.arange(len(held)), pos_kept)
            printed = []
            for q, pos in held.by_query():
                for p in pos[show[pos]]:
                    out.write("%s,%d,%s,%r%s\n" % (heads[q], int(held.rank[p]) + 1, t_cols(held.t[p]), float(held.f[p]), more[p]))
                    printed.append(int(p))
            if a.paf is not None:
                write_paf(held, printed)
        return 0
    if a.heuristic:
        if a.kd is None or a.r_squared is None:
            ap.error("--heuristic needs --kd and --r-squared")
        if a.global_ or a.f_min is not None:
            ap.error("--heuristic is the local loop over all pairs: no --global, no --f-min")
        from .heuristic import align_set
        from .simple import Heuristics
        codes = encode_records(records, alphabet)
        v = alphabet.volume()
        if a.frequencies is not None:
            freq = np.array([float(x) for x in a.frequencies.split(",")], dtype=np.float64)
            if len(freq) != v:
                ap.error("--frequencies: %d values, one per code of the alphabet" % v)
        else:
            every = np.concatenate([np.asarray(c, dtype=np.uint8) for c in codes])
            every = every[every < v]
            freq = np.bincount(every, minlength=v).astype(np.float64) / max(len(every), 1)
        with SeqSet(codes, alphabet, device=a.device) as ss:
            for _, q, t, r in align_set(ss, a.del_, a.ext, matrix, Heuristics(kd=a.kd, r_squared=a.r_squared, frequencies=freq)):
                out.write("%s,%s,%s\n" % (heads[q], heads[t], repr(float(r.alignment.f)) if not isinstance(r, Exception) else "panic: %s" % r))
        return 0
    with make_set(encode_records(records, alphabet)) as ss:
        if a.kmer is not None:
            cand = candidates(ss, square(ss) if a.both_strands else None)
        if a.kmer is not None and a.f_min is None:
            f, status = cand.score(matrix, a.del_, a.ext, semantics=sem)
            for c in (np.flatnonzero(once(cand.q, cand.t)) if a.both_strands else range(len(cand))):
                out.write("%s,%s,%s,%d%s\n" % (heads[int(cand.q[c])], t_cols(cand.t[c]),
                                               repr(float(f[c])) if status[c] == _ffi.OK else _ffi.STATUS_NAMES[int(status[c])], int(cand.shared[c]),
                                               (",%d" % int(cand.diag[c]) if a.seed_join else "") +
                                               (",%d,%d,%d,%d,%d,%d" % tuple(int(cand.chain[c][n]) for n in ("score", "anchors", "q_start", "q_end", "t_start", "t_end"))
                                                if a.chain else "")))
        elif a.f_min is None and a.both_strands:
            f, status = ss.score(matrix, a.del_, a.ext, square(ss), semantics=sem)
            for i in range(n_rec):
                for t in range(2 * n_rec):
                    if i < t % n_rec:
                        k = i * 2 * n_rec + t
                        out.write("%s,%s,%s\n" % (heads[i], t_cols(t), repr(float(f[k])) if status[k] == _ffi.OK else _ffi.STATUS_NAMES[int(status[k])]))
        elif a.f_min is None:
            f, status = ss.score(matrix, a.del_, a.ext, None, semantics=sem)
            k = 0
            for i in range(len(heads)):
                for j in range(i + 1, len(heads)):
                    out.write("%s,%s,%s\n" % (heads[i], heads[j], repr(float(f[k])) if status[k] == _ffi.OK else _ffi.STATUS_NAMES[int(status[k])]))
                    k += 1
        else:
            held = cand.hits(matrix, a.del_, a.ext, a.f_min, semantics=sem) if a.kmer is not None else \
                ss.hits(matrix, a.del_, a.ext, a.f_min, square(ss) if a.both_strands else None, semantics=sem)
            if a.cluster is not None:
                clustered(held)
                return 0
            pos_kept, reports = kept(held)
            if a.both_strands:                        # the rectangle holds every pair from both sides: the rows are one side's
                pos_kept = np.arange(len(held), dtype=np.uint32) if pos_kept is None else np.asarray(pos_kept, dtype=np.uint32)
                side = once(held.q[pos_kept], held.t[pos_kept])
                pos_kept, reports = pos_kept[side], (None if reports is None else reports[side])
            more = tail(held, pos_kept, reports)
            for h in (range(len(held)) if pos_kept is None else pos_kept):
                out.write("%s,%s,%r%s\n" % (heads[int(held.q[h])], t_cols(held.t[h]), float(held.f[h]), more[int(h)]))
            if a.paf is not None:
                write_paf(held, np.arange(len(held)) if pos_kept is None else pos_kept)
    return 0


if __name__ == "__main__":
    sys.exit(main())
