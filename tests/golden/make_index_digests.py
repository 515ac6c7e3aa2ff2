#!/usr/bin/env python3
"""Generate tests/golden/ref_index_sha256.json: the SHA-256 digests of the five index files <fa>.gnumap.{pac,ann,amb,bwt,sa}
that the REFERENCE's own bwa_index (via oracle/_ref) writes for the inputs of tests/test_index_build.py (seeded random genomes,
FASTA edge cases) and for the real-sequence fixture tests/golden/celgen/celgen.fa.gz.  Run where oracle/_ref can be built:
    python tests/golden/make_index_digests.py
"""
import gzip
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from reflib import RefLib, have_ref                                                  # noqa: E402
from test_index_build import FASTA_EDGE_CASES, RANDOM_GENOMES, _write_random_fasta, digests, text_key   # noqa: E402


def ref_build(fa):
    assert RefLib().index_build(fa) == 0
    return digests(fa)


def main():
    if not have_ref():
        raise SystemExit("oracle/_ref/libgnumap_ref.so is missing: make -C oracle ref")
    out = {"random_genomes": {}, "fasta_edge_cases": {}, "celgen": {}}
    with tempfile.TemporaryDirectory() as d:
        for seed, spec in RANDOM_GENOMES:
            fa = os.path.join(d, f"random{seed}.fa")
            _write_random_fasta(fa, np.random.default_rng(seed), spec)
            out["random_genomes"][str(seed)] = ref_build(fa)
        for i, text in enumerate(FASTA_EDGE_CASES):
            fa = os.path.join(d, f"edge{i}.fa")
            open(fa, "wb").write(text)
            out["fasta_edge_cases"][text_key(text)] = ref_build(fa)
        fa = os.path.join(d, "celgen.fa")
        with gzip.open(os.path.join(HERE, "celgen", "celgen.fa.gz"), "rb") as f, open(fa, "wb") as o:
            shutil.copyfileobj(f, o)
        out["celgen"]["celgen.fa"] = ref_build(fa)
    with open(os.path.join(HERE, "ref_index_sha256.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
