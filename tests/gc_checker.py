"""The GC column of getBamCounts' referenceFasta block (reference R/countBamInGranges.R:333-344), restated in plain Python on the sequence as a
string: slice the target, upper-case it (a DNAString holds upper case), count G + C and A + T + G + C, divide, NA (NaN) where the second is
zero.  Not a run of the reference: there is no Bioconductor here.  Also a small FASTA writer for the tests."""
import numpy as np


def gc_counts(seqs, chromosome, start, end):
    """int (gc, atgc) per target; seqs: {name: sequence string}; start, end 1-based, both included"""
    gc, atgc = [], []
    for c, s, e in zip(chromosome, start, end):
        x = seqs[str(c)][int(s) - 1:int(e)].upper()
        assert len(x) == int(e) - int(s) + 1, "target beyond its sequence"
        g = x.count("G") + x.count("C")
        gc.append(g)
        atgc.append(g + x.count("A") + x.count("T"))
    return np.asarray(gc, dtype=np.int64), np.asarray(atgc, dtype=np.int64)


def gc_fraction(seqs, chromosome, start, end):
    gc, atgc = gc_counts(seqs, chromosome, start, end)
    out = np.full(gc.size, np.nan)
    np.divide(gc, atgc, out=out, where=atgc > 0)
    return out


def widened(seqs, chromosome, start, end, flank):
    """the targets widened by `flank` bases on both sides, clipped to their sequences"""
    length = np.asarray([len(seqs[str(c)]) for c in chromosome], dtype=np.int64)
    return np.maximum(np.asarray(start, dtype=np.int64) - flank, 1), np.minimum(np.asarray(end, dtype=np.int64) + flank, length)


def fasta_bytes(records, width, eol=b"\n", final_eol=True):
    """(the file's bytes, its .fai records [(name, length, offset, line_bases, line_width)]) for records [(header text, sequence)] written `width`
    bases a line.  The expected index is written down from the layout as it is laid, not computed by the code under test."""
    out, fai = bytearray(), []
    for k, (header, seq) in enumerate(records):
        out += b">" + header.encode() + eol
        offset = len(out)
        lines = [seq[i:i + width] for i in range(0, len(seq), width)]
        for j, line in enumerate(lines):
            out += line.encode()
            if final_eol or not (k == len(records) - 1 and j == len(lines) - 1):
                out += eol
        first_width = 0
        if lines:
            first_width = len(lines[0]) + len(eol) if (len(lines) > 1 or final_eol or k < len(records) - 1) else len(lines[0])
        fai.append((header.split()[0], len(seq), offset, len(lines[0]) if lines else 0, first_width))
    return bytes(out), fai


def random_sequence(rng, n, alphabet="ACGTacgtNnRYSWKM"):
    return "".join(rng.choice(list(alphabet), size=n))
