"""exomedepth_amd/fasta.py on the host: the index built from a file equals the .fai written down by hand, byte_range() addresses exactly the bases
asked for, and every refusal is raised."""
import gzip

import numpy as np
import pytest

import gc_checker as gck
from exomedepth_amd.fasta import FastaIndex

WIDTHS = [1, 7, 60, 61]


def _write(tmp_path, data, name="ref.fa"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_index_by_hand(tmp_path):
    """three records typed out, with descriptions, a short last line, CRLF in one file and no final line end in the other"""
    lf = b">chr1 first sequence\nACGTACG\nTTGACCA\nGG\n>chr2\tdescription=2\nNNNNNNN\nAC\n>3 x\nA"
    idx = FastaIndex(_write(tmp_path, lf))
    assert idx.records == [("chr1", 16, 21, 7, 8), ("chr2", 9, 60, 7, 8), ("3", 1, 76, 1, 1)]
    assert idx.names == ["chr1", "chr2", "3"] and len(idx) == 3 and not idx.from_fai
    crlf = b">a b c\r\nACGT\r\nAC\r\n>b\r\nGGGG\r\nGGGG\r\n"
    idx = FastaIndex(_write(tmp_path, crlf, "crlf.fa"))
    assert idx.records == [("a", 6, 8, 4, 6), ("b", 8, 22, 4, 6)]
    first, last = idx.byte_range("a", [1, 4, 5], [4, 6, 6])
    assert [crlf[a:b] for a, b in zip(first, last)] == [b"ACGT", b"T\r\nAC", b"AC"]
    assert first.dtype == np.int64 and last.dtype == np.int64


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("final_eol", [True, False])
@pytest.mark.parametrize("width", WIDTHS)
def test_built_index_equals_the_layout(tmp_path, width, eol, final_eol):
    rng = np.random.default_rng(width)
    records = [("s1 a description", gck.random_sequence(rng, 3 * width)),           # a full last line
               ("s2\tmore words here", gck.random_sequence(rng, 5 * width + max(1, width // 2) if width > 1 else 5)),   # a short one
               ("s3", gck.random_sequence(rng, 1)),
               ("s4 |x|", gck.random_sequence(rng, 200))]
    data, fai = gck.fasta_bytes(records, width, eol, final_eol)
    path = _write(tmp_path, data)
    idx = FastaIndex(path)
    assert idx.records == fai
    # the same records read back from a .fai file, which is checked against the FASTA file and accepted
    idx.write_fai()
    again = FastaIndex(path)
    assert again.from_fai and again.records == fai
    text = open(path + ".fai").read().splitlines()
    assert text == ["%s\t%d\t%d\t%d\t%d" % r for r in fai]


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("width", WIDTHS)
def test_byte_range_every_pair(tmp_path, width, eol):
    """every (start, end) of a 200-base sequence: the file's bytes [first, last_excl) without their line ends are the bases start .. end"""
    rng = np.random.default_rng(100 + width)
    seq = gck.random_sequence(rng, 200)
    lead = gck.random_sequence(rng, 33)
    data, _ = gck.fasta_bytes([("lead in", lead), ("s desc", seq), ("tail", "ACGT")], width, eol)
    idx = FastaIndex(_write(tmp_path, data))
    s, e = np.triu_indices(200)
    first, last = idx.byte_range("s", s + 1, e + 1)
    assert first.size == 200 * 201 // 2
    for a, b, lo, hi in zip(s.tolist(), e.tolist(), first.tolist(), last.tolist()):
        got = data[lo:hi].replace(b"\r", b"").replace(b"\n", b"")
        assert got == seq[a:b + 1].encode(), (a + 1, b + 1)
        assert data[lo:lo + 1] == seq[a].encode() and data[hi - 1:hi] == seq[b].encode()      # no line end at either edge
    # names per range, sequences mixed
    first, last = idx.byte_range(["tail", "s", "lead"], [1, 200, 33], [4, 200, 33])
    assert [data[a:b].replace(b"\r", b"").replace(b"\n", b"") for a, b in zip(first, last)] == [b"ACGT", seq[199:].encode(), lead[32:].encode()]


def test_refusals(tmp_path):
    with pytest.raises(ValueError, match="different length"):
        FastaIndex(_write(tmp_path, b">a\nACGT\nACG\nACGT\n", "unequal.fa"))
    with pytest.raises(ValueError, match="different length"):
        FastaIndex(_write(tmp_path, b">a\nACGT\nACGT\r\nAC\n", "mixed_eol.fa"))
    with pytest.raises(ValueError, match="longer"):
        FastaIndex(_write(tmp_path, b">a\nACGT\nACGTA\n", "long_last.fa"))
    with pytest.raises(ValueError, match="blank line inside sequence 'a'"):
        FastaIndex(_write(tmp_path, b">a x\nACGT\n\nACGT\n", "blank.fa"))
    with pytest.raises(ValueError, match="'b' occurs twice"):
        FastaIndex(_write(tmp_path, b">b 1\nAC\n>a\nAC\n>b 2\nAC\n", "dup.fa"))
    with pytest.raises(ValueError, match="before the first"):
        FastaIndex(_write(tmp_path, b"ACGT\n>a\nAC\n", "stray.fa"))
    # blank lines after a sequence's last line are not inside it
    assert FastaIndex(_write(tmp_path, b">a\nACGT\nAC\n\n>b\nAC\n\n", "trailing.fa")).records == [("a", 6, 3, 4, 5), ("b", 2, 15, 2, 3)]
    assert FastaIndex(_write(tmp_path, b"", "empty.fa")).records == []
    assert FastaIndex(_write(tmp_path, b">a\n>b\nAC\n", "empty_seq.fa")).records == [("a", 0, 3, 0, 0), ("b", 2, 6, 2, 3)]

    gz = tmp_path / "ref.fa.gz"
    with gzip.open(gz, "wb") as f:
        f.write(b">a\nACGT\n")
    with pytest.raises(ValueError, match="compressed"):
        FastaIndex(str(gz))

    good = b">a\nACGT\nACGT\n>b\nGGCC\nGG\n"
    path = _write(tmp_path, good, "stale.fa")
    for fai, who in [("a\t8\t3\t4\t5\nb\t6\t17\t4\t5\n", "'b'"),          # b's offset points into its first line: no line end before it
                     ("a\t8\t3\t4\t5\nb\t60\t16\t4\t5\n", "'b'"),         # b's last base would lie beyond the file
                     ("a\t8\t4\t4\t5\nb\t6\t16\t4\t5\n", "'a'")]:
        open(path + ".fai", "w").write(fai)
        with pytest.raises(ValueError, match="stale.*%s" % who):
            FastaIndex(path)
    open(path + ".fai", "w").write("a\t8\t3\t4\t5\nb\t6\t16\t4\t5\n")
    idx = FastaIndex(path)
    assert idx.from_fai and idx.records == [("a", 8, 3, 4, 5), ("b", 6, 16, 4, 5)]
    with pytest.raises(ValueError, match="beyond the 6 bases of sequence 'b'"):
        idx.byte_range("b", 1, 7)
    with pytest.raises(ValueError, match="beyond the 8 bases of sequence 'a'"):
        idx.byte_range(["b", "a"], [1, 8], [6, 9])
    with pytest.raises(ValueError, match="'c' is not in"):
        idx.byte_range("c", 1, 2)
    with pytest.raises(ValueError, match="1 <= start <= end"):
        idx.byte_range("a", 0, 2)
    with pytest.raises(ValueError, match="1 <= start <= end"):
        idx.byte_range("a", 3, 2)
