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
"""
import argparse
import sys

from . import _ffi
from .enums import DNA, Protein
from .fasta import encode_records, read_fasta
from .matrices import get_blosum62, nucleotide_matrix
from .seqset import SeqSet


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
    a = ap.parse_args(argv)
    records = read_fasta(a.input)
    if len(records) < 2:
        ap.error("%s: an all-against-all run needs two or more records" % a.input)
    alphabet = DNA if a.dna else Protein
    matrix = nucleotide_matrix() if a.dna else get_blosum62()
    sem = _ffi.CORE_GLOBAL if a.global_ else _ffi.CORE_LOCAL
    heads = [r.head.decode("utf-8", "replace") for r in records]
    out = sys.stdout
    if a.best is not None:
        if a.heuristic:
            ap.error("--best selects by the score of the plain alignment: not with --heuristic")
        if not 1 <= a.best <= _ffi.SEQSET_BEST_MAX:
            ap.error("--best: K must lie in 1 .. %d" % _ffi.SEQSET_BEST_MAX)
        with SeqSet(encode_records(records, alphabet), alphabet, device=a.device) as ss:
            held = ss.best(matrix, a.del_, a.ext, a.best, f_min=float("-inf") if a.f_min is None else a.f_min, skip_self=True, semantics=sem)
            for q, pos in held.by_query():
                for p in pos:
                    out.write("%s,%d,%s,%r\n" % (heads[q], int(held.rank[p]) + 1, heads[int(held.t[p])], float(held.f[p])))
        return 0
    if a.heuristic:
        if a.kd is None or a.r_squared is None:
            ap.error("--heuristic needs --kd and --r-squared")
        if a.global_ or a.f_min is not None:
            ap.error("--heuristic is the local loop over all pairs: no --global, no --f-min")
        import numpy as np
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
    with SeqSet(encode_records(records, alphabet), alphabet, device=a.device) as ss:
        if a.f_min is None:
            f, status = ss.score(matrix, a.del_, a.ext, None, semantics=sem)
            k = 0
            for i in range(len(heads)):
                for j in range(i + 1, len(heads)):
                    out.write("%s,%s,%s\n" % (heads[i], heads[j], repr(float(f[k])) if status[k] == _ffi.OK else _ffi.STATUS_NAMES[int(status[k])]))
                    k += 1
        else:
            held = ss.hits(matrix, a.del_, a.ext, a.f_min, None, semantics=sem)
            for q, t, f in zip(held.q, held.t, held.f):
                out.write("%s,%s,%r\n" % (heads[int(q)], heads[int(t)], float(f)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
