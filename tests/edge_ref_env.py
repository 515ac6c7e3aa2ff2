"""How the edge fixtures' reference runs are started (tests/golden/make_edge_fixtures.py and the re-run check of tests/test_edge_cpu.py).

The reference takes its coverage arrays from malloc and adds to them without clearing them first (GenomeBwt.cpp:323).  For a genome of a
few hundred kbp malloc hands out fresh zero pages; for the 10 kbp edge genome the arrays are a few kB of recycled heap, and the track text
is whatever was there before (the SAM text does not depend on it).  With this glibc setting every allocation is a mapping of its own, that
is zero pages, as it is for a larger genome: the program is still the unmodified one, and it then writes the same bytes in every run.  The
committed .sgr / .gmp files are therefore the reference's tracks on zeroed arrays, not what a bare run on this genome happens to print."""
REF_MALLOC_ENV = {"MALLOC_MMAP_THRESHOLD_": "0"}
