"""What --sam_sort=coordinate has to write, as a plain Python model: SAM text in, SAM text out.

* header lines ('@') stay where they are and in their order, behind a first line `@HD VN:1.0 SO:coordinate`;
* rows are sorted STABLY by (rank of RNAME among the @SQ lines, POS as an integer): equal keys keep input order;
* rows whose RNAME is '*' go last, in input order.

`text` may be str or bytes; the result has the same type.  sort_rows() is the same rule for bare rows and a list of contig names
(the ABI tests have no header)."""

HD = "@HD\tVN:1.0\tSO:coordinate\n"


def row_key(row, rank):
    """(contig rank, position) of a row (one line, str); rows without a contig sort behind every contig"""
    f = row.split("\t")
    if f[2] == "*":
        return (len(rank), 0)
    return (rank[f[2]], int(f[3]))


def sort_rows(rows, contigs):
    """rows: list of lines (str, with or without '\\n'); contigs: names in @SQ order"""
    rank = {c: i for i, c in enumerate(contigs)}
    return sorted(rows, key=lambda r: row_key(r, rank))          # sorted() is stable


def sam_sort_model(text):
    is_bytes = isinstance(text, (bytes, bytearray))
    t = bytes(text).decode("latin-1") if is_bytes else text
    lines = t.splitlines(keepends=True)
    header = [l for l in lines if l.startswith("@")]
    rows = [l for l in lines if not l.startswith("@")]
    contigs = [f[3:].rstrip("\n") for l in header if l.startswith("@SQ") for f in l.split("\t") if f.startswith("SN:")]
    out = "".join([HD] + [l for l in header if not l.startswith("@HD")] + sort_rows(rows, contigs))
    return out.encode("latin-1") if is_bytes else out
