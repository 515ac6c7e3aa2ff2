#!/usr/bin/env python3
"""FASTA read fixtures, produced by the UNMODIFIED reference program and the unmodified reference functions.

Run in the build container only (needs the reference sources):
    make -C oracle ref refbin && python tests/golden/make_fasta_fixtures.py

Inputs written (deterministic, derived from the committed syn.fq; our own generator):

    syn_reads.fa       the reads of syn.fq (8 .. 150 bp) as FASTA: a fifth of the records in lower case; a third split over two sequence
                       lines and every seventh over three; every sixth name with a description behind a space (the reference prints the
                       whole header line); every tenth read with a run of 2 .. 5 n; about a quarter of the reads with one to four of the
                       ten other IUPAC letters (r y k m s w b d h v, both cases, cycled so that each of the twenty characters occurs
                       many times), half of them compatible with the base they replace; the 8-, 10- and 11-bp reads stay shorter than -m
    syn_reads_u100.fa  200 of the 100-bp reads, every second one with one to three ambiguity codes: a block of ONE length

Outputs committed:

    tests/golden/ref_runs_fasta/<mode>.sam.gz            the reference program's SAM file (-c 1), @PG line dropped
    tests/golden/ref_runs_fasta/<mode>.sgr.gz|.gmp.gz    its coverage / per-nucleotide track text
    tests/golden/ref_runs_fasta/manifest.json            argv and read file per mode
    tests/golden/fasta_vectors.npz                       function-level vectors through oracle/_ref/libgnumap_ref.so, whose harness takes
                                                         arbitrary PWM rows: self score, NW score (fp32 bits), traceback (aligned string,
                                                         length, CIGAR) of (read, strand, window) triples at true loci and at decoys

Everything committed is DATA (our inputs, the reference's outputs on them); no reference source text.
"""
import gzip, json, os, shutil, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from fasta_model import AMBIGUITY, IUPAC, parse_fasta, pwm_rows        # tests/fasta_model.py: the rows handed to the reference's functions
REFBIN = os.path.join(ROOT, "oracle", "_ref", "gnumap_ref")
OUT = os.path.join(HERE, "ref_runs_fasta")

# name -> (reference argv between "-a 0.9" and the read file, read file)
MODES = {
    "default":  ([], "syn_reads.fa"),
    "all_a80":  (["--print_all_sam", "-a", "0.8"], "syn_reads.fa"),
    "no_nw":    (["--no_nw"], "syn_reads.fa"),
    "bs":       (["-b"], "syn_reads.fa"),
    "b2":       (["--b2"], "syn_reads.fa"),
    "atog":     (["-d"], "syn_reads.fa"),
    "m14_j7":   (["-m", "14", "-j", "7"], "syn_reads.fa"),
    "M5":       (["-M", "5"], "syn_reads.fa"),
    "M1":       (["-M", "1"], "syn_reads.fa"),
    "up":       (["--up_strand"], "syn_reads.fa"),
    "down":     (["--down_strand"], "syn_reads.fa"),
    "q60":      (["-q", "60"], "syn_reads.fa"),
    "raw60":    (["-r", "-a", "60"], "syn_reads.fa"),
    "T2":       (["-T", "2"], "syn_reads.fa"),
    "u":        (["-u", "1"], "syn_reads.fa"),                 # -u swallows the next argv (Driver.cpp:2768-2770)
    "h30":      (["-h", "30"], "syn_reads.fa"),
    "subst":    (["-S", "subst.txt"], "syn_reads.fa"),
    "bin1":     (["--bin_size=1"], "syn_reads.fa"),
    "u100":     ([], "syn_reads_u100.fa"),
}
CODES = [c for pair in zip(AMBIGUITY, AMBIGUITY.upper()) for c in pair]         # r R y Y ...


def read_fastq(path):
    recs = []
    with open(path, "rb") as f:
        while True:
            name = f.readline()
            if not name:
                break
            seq = f.readline().rstrip(b"\n"); f.readline(); f.readline()
            recs.append((name[1:].rstrip(b"\n"), seq))
    return recs


class Coder:
    """puts ambiguity codes into a sequence; the twenty characters are handed out in turn"""
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed); self.turn = 0

    def code_for(self, base, compatible):
        for _ in range(len(CODES)):
            c = CODES[self.turn % len(CODES)]; self.turn += 1
            if (chr(base).lower() in IUPAC[c.lower()]) == compatible or chr(base).lower() not in "acgt":
                return ord(c)
        return ord(c)

    def put(self, seq, count):
        s = bytearray(seq)
        for k, pos in enumerate(sorted(self.rng.choice(len(s), min(count, len(s)), replace=False))):
            s[pos] = self.code_for(s[pos], compatible=(k + self.turn) % 2 == 0)
        return bytes(s)


def write_fasta(path, recs, split=True):
    with open(path, "wb") as f:
        for i, (name, seq) in enumerate(recs):
            f.write(b">" + name + b"\n")
            pieces = 3 if (split and i % 7 == 0 and len(seq) >= 9) else 2 if (split and i % 3 == 0 and len(seq) >= 9) else 1
            cut = [len(seq) * k // pieces for k in range(pieces + 1)]
            for a, b in zip(cut, cut[1:]):
                f.write(seq[a:b] + b"\n")


def make_reads(base):
    coder = Coder(20240917)
    rng = np.random.default_rng(5)
    out = []
    for i, (name, seq) in enumerate(base):
        s = seq
        if i % 4 == 1 and len(s) >= 20:
            s = coder.put(s, 1 + (i // 4) % 4)
        if i % 10 == 3 and len(s) >= 30:
            a = int(rng.integers(0, len(s) - 6)); k = 2 + i % 4
            s = s[:a] + (b"n" if i % 20 == 3 else b"N") * k + s[a + k:]
        if i % 5 == 2:
            s = s.lower()
        if i % 6 == 1:
            name = name + b" sample " + str(i).encode() + b" lane=3"
        assert len(s) == len(seq)
        out.append((name, s))
    return out


def make_u100(base):
    coder = Coder(77)
    pick = [r for r in base if len(r[1]) == 100][:200]
    assert len(pick) == 200
    return [(n, coder.put(s, 1 + k % 3) if k % 2 else s) for k, (n, s) in enumerate(pick)]


def contig_offsets(fa):
    names, lens = [], []
    for line in open(fa, "rb"):
        if line.startswith(b">"):
            names.append(line[1:].split()[0].decode()); lens.append(0)
        else:
            lens[-1] += len(line.strip())
    return names, np.cumsum([0] + lens)


def make_vectors(recs):
    from reflib import RefLib, revcomp_pwm, revcomp_str
    ref = RefLib()
    ref.setup(0)
    fa = os.path.join(HERE, "syn.fa")
    ix = ref.index_load(fa)
    names, offs = contig_offsets(fa)
    l_pac = int(offs[-1])
    rng = np.random.default_rng(99)
    # reads of 24 .. 150 bp: every read that carries an ambiguity code or n, and a share of the plain ones
    reads = [(n, s) for k, (n, s) in enumerate(recs) if 24 <= len(s) <= 150 and (any(chr(c).lower() not in "acgt" for c in s) or k % 5 == 0)]
    seen = set(chr(c) for _, s in reads for c in s)
    assert all(c in seen and c.upper() in seen for c in IUPAC), sorted(seen)
    self_score = np.array([ref.self_score(pwm_rows(s), s) for _, s in reads], np.float32)
    cases = []
    for r, (n, s) in enumerate(reads):
        L = len(s)
        parts = n.split(b" ")[0].decode().split("_")
        for t in range(2):
            b = int(rng.integers(0, l_pac - L))                               # a decoy
            rc = int(rng.integers(0, 2))
            if t == 0 and len(parts) == 5 and parts[0].startswith("r") and parts[1] in names:
                b = int(offs[names.index(parts[1])]) + int(parts[2]) + int(rng.integers(-2, 3))
                b = max(0, min(b, l_pac - L))
                rc = 1 if parts[3] == "-" else 0
            w = ref.window(ix, b, L)
            if w:
                cases.append((r, b, rc, w))
    nw = np.zeros(len(cases), np.float32); tb_len = np.zeros(len(cases), np.int32); tb_al = []; tb_cg = []
    for k, (r, b, rc, w) in enumerate(cases):
        s = reads[r][1]
        P, cons = pwm_rows(s), s
        if rc:
            P, cons = revcomp_pwm(P), revcomp_str(cons)
        nw[k] = ref.nw_score(P, w)
        al, alen, cg = ref.traceback(P, cons, w)
        tb_al.append(al); tb_cg.append(cg); tb_len[k] = alen
    table, gap, maxgap = ref.get_scores()
    vec = dict(read_seq=np.array([s for _, s in reads], dtype="S160"), self_score=self_score,
               nw_read=np.array([c[0] for c in cases], np.int32), nw_begin=np.array([c[1] for c in cases], np.uint64),
               nw_rc=np.array([c[2] for c in cases], np.int8), nw_window=np.array([c[3] for c in cases], dtype="S160"), nw_score=nw,
               tb_aligned_hex=np.array([a.hex() for a in tb_al], dtype="S700"), tb_len=tb_len, tb_cigar=np.array(tb_cg, dtype="S256"),
               S=table, gap=np.float32(gap), max_gap=np.int32(maxgap))
    np.savez_compressed(os.path.join(HERE, "fasta_vectors.npz"), **vec)
    true_loci = sum(1 for k, c in enumerate(cases) if nw[k] > 0.5 * self_score[c[0]])
    print(f"fasta_vectors.npz: {len(reads)} reads, {len(cases)} (read, strand, window) triples, {true_loci} of them at a true locus")
    assert len(cases) >= 300 and true_loci >= 100


def coded(seq):
    return any(c in seq for c in AMBIGUITY + AMBIGUITY.upper())


def main():
    assert os.path.exists(REFBIN), "make -C oracle ref refbin first"
    os.makedirs(OUT, exist_ok=True)
    base = read_fastq(os.path.join(HERE, "syn.fq"))
    recs = make_reads(base)
    write_fasta(os.path.join(HERE, "syn_reads.fa"), recs)
    write_fasta(os.path.join(HERE, "syn_reads_u100.fa"), make_u100(base), split=False)
    assert parse_fasta(open(os.path.join(HERE, "syn_reads.fa"), "rb").read()) == recs
    if "--vectors-only" not in sys.argv:
        work = tempfile.mkdtemp()
        for f in os.listdir(HERE):
            if f.startswith("syn.") or f.startswith("syn_reads") or f == "subst.txt":
                shutil.copy(os.path.join(HERE, f), work)
        manifest = {}
        for name, (args, fa) in MODES.items():
            r = subprocess.run([REFBIN, "-g", "syn.fa", "-o", name, "-a", "0.9", "-c", "1"] + args + [fa], cwd=work, capture_output=True, text=True)
            assert r.returncode == 0, (name, r.stderr[-2000:])
            sam = [l for l in open(os.path.join(work, name + ".sam"), "rb") if not l.startswith(b"@PG")]
            with gzip.GzipFile(os.path.join(OUT, name + ".sam.gz"), "wb", mtime=0) as g:
                g.write(b"".join(sam))
            tracks = []
            for ext in ("sgr", "gmp"):
                p = os.path.join(work, name + "." + ext)
                if os.path.exists(p):
                    with gzip.GzipFile(os.path.join(OUT, name + "." + ext + ".gz"), "wb", mtime=0) as g:
                        g.write(open(p, "rb").read())
                    tracks.append(ext)
            rows = [l.split(b"\t") for l in sam if not l.startswith(b"@")]
            n_code = sum(1 for f in rows if coded(f[9].decode())); n_n = sum(1 for f in rows if b"n" in f[9].lower())
            # a minus-strand row prints reverse_comp's string, where every code is 'n': count the coded reads by name there
            by_name = {n: s for n, s in parse_fasta(open(os.path.join(HERE, fa), "rb").read())}
            coded_rows = [f for f in rows if coded(by_name[f[0]].decode())]
            n_rows = [f for f in rows if b"n" in by_name[f[0]].lower()]
            strands = {f[1] for f in coded_rows}, {f[1] for f in n_rows}
            manifest[name] = dict(argv=args, fasta=fa, sam_lines=len(sam), records=len(rows), tracks=tracks,
                                  records_of_coded_reads=len(coded_rows), records_of_n_reads=len(n_rows))
            print(f"{name:10s} {len(rows):5d} records, {len(coded_rows):4d} of reads with an ambiguity code ({n_code} print one), {len(n_rows):4d} of reads with n ({n_n} rows hold n)  {tracks}")
            assert len(rows) >= 100, name                                   # no vacuous mode
            if name == "default":                                           # ambiguity codes and n reach the output, on both strands
                seq_rows = [f for f in rows if coded(f[9].decode()) or b"n" in f[9].lower()]
                assert n_code >= 40 and n_n >= 20 and {f[1] for f in seq_rows} == {b"0", b"16"}, (n_code, n_n)
                assert strands[0] == {b"0", b"16"} and strands[1] == {b"0", b"16"}, strands
        json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
        shutil.rmtree(work)
    make_vectors(recs)


if __name__ == "__main__":
    main()
