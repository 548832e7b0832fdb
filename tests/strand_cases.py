"""The inputs of the strand tests (tests/test_strand_gpu.py), built once here so that a test without a GPU can assert from the oracle alone
what they are built for (tests/test_strand_rules_cpu.py)."""
import numpy as np

from aligner_amd.enums import DNA

# lengths at the edges of the mirror kernel's 16-byte chunks and 4 KiB tiles, ordered so that the offsets are unaligned
MIRROR_LENGTHS = (1, 17, 0, 2, 15, 63, 16, 65, 64, 255, 257, 256, 4095, 4097, 4096)
F_MIN = 560.0                 # of the parity set's held passes: random nucleotide records of these lengths reach a few hundred under 10 / 1
DEL, EXT = 10.0, 1.0


def odd_table():
    """a byte table that is a bijection and no involution"""
    return ((np.arange(256) * 7 + 3) & 255).astype(np.uint8)


def mirror_records():
    rng = np.random.default_rng(31)
    recs = [rng.integers(0, 256, size=n).astype(np.uint8) for n in MIRROR_LENGTHS]
    recs[-2][:256] = np.arange(256, dtype=np.uint8)          # every byte value, whatever the generator drew
    return recs


def revcomp(codes):
    return DNA.complement_map()[np.asarray(codes, dtype=np.uint8)[::-1]]


A, B, PAL, NEAR = 2, 7, 4, 9  # positions in parity_records()


def parity_records():
    """12 nucleotide records of 40 to 300 residues: B is the reverse complement of A with three substitutions, PAL is its own reverse
    complement, NEAR is A with two substitutions between flanks (a hit on the plus strand); the rest is random."""
    rng = np.random.default_rng(77)
    lengths = [40, 300, 120, 97, 60, 151, 64, 120, 255, 150, 43, 200]
    recs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in lengths]
    b = revcomp(recs[A]).copy()
    for at in (11, 60, 101):
        b[at] = (b[at] + 1) % 4
    recs[B] = b
    half = rng.integers(0, 4, size=30).astype(np.uint8)
    recs[PAL] = np.concatenate([half, revcomp(half)])
    near = recs[A].copy()
    near[[30, 90]] = (near[[30, 90]] + 2) % 4
    recs[NEAR] = np.concatenate([rng.integers(0, 4, size=13), near, rng.integers(0, 4, size=17)]).astype(np.uint8)
    assert [len(r) for r in recs] == lengths and np.array_equal(revcomp(recs[PAL]), recs[PAL])
    return recs


COLUMNS = (1, 63, 64, 65, 129)


def cigar_records():
    """15 nucleotide records: prefixes of one random sequence -- a prefix of c residues against the prefix of c + 1 aligns in exactly c
    columns without a gap, c in COLUMNS -- and copies of the longest with an insert, a deletion and both, whose alignments carry gap
    runs, a suffix, and the reverse complements of the prefixes of c + 1 residues, so that the same c columns come about between a record
    and a mirror; in a global pass the prefixes against the longer records end with a gap run and the suffix begins with one."""
    rng = np.random.default_rng(1234)
    other = rng.integers(0, 4, size=131).astype(np.uint8)
    recs = [other[:n].copy() for n in (1, 2, 63, 64, 65, 66, 129, 130)]
    recs.append(np.insert(other[:130], 40, (other[40:44] + 1) % 4).astype(np.uint8))
    recs.append(np.delete(np.insert(other[:130], 100, (other[100:103] + 2) % 4), np.arange(20, 25)).astype(np.uint8))
    first = next(a for a in range(66, 130) if other[a] != other[0] and other[a + 1] != other[0])    # (its head cannot pair with the prefixes' head)
    recs.append(other[first:130].copy())
    recs += [revcomp(other[:c + 1]) for c in COLUMNS[1:]]
    return recs


def command_records():
    """(heads, sequences as text): six records with one planted opposite-strand pair -- record 1 begins with a core of 80 and ends in a
    flank of A, record 4 holds the core's reverse complement between flanks of G, so that on the minus strand the core aligns and nothing
    beside it can.  The reference's local alignment starts where its running score is exactly 0; the core at the very start of record 1
    makes that the border: q 0 .. 80 of record 1 (110 residues), t 15 .. 95 of record 4 (120 residues), 80 matches in 80 columns,
    f = 400 under 5 / -4."""
    rng = np.random.default_rng(9)
    core = rng.integers(0, 4, size=80).astype(np.uint8)
    a, g = np.zeros(1, dtype=np.uint8), np.full(1, 3, dtype=np.uint8)
    recs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (90, 0, 70, 101, 0, 85)]
    recs[1] = np.concatenate([core, np.repeat(a, 30)])
    recs[4] = np.concatenate([np.repeat(g, 15), revcomp(core), np.repeat(g, 25)])
    return ["r%d desc" % i for i in range(6)], [DNA.vec_to_str(r) for r in recs]
