"""Test helper: a NumPy / math restatement of the SNP statistic the product computes on the device (gnumap_amd/csrc/gm_snpcall.hip), i.e.
GenomeBwt::is_snp / LRT / dipLRT / PrintSNPCall (src/GenomeBwt.cpp:739-901, 1011-1090) with gsl_cdf_chisq_P in closed form, the likelihood
ratios kept as logarithms and the forced-monoploid case defined as dip = false, p = pval1.  Own code; the numbers it is held to come from
the unmodified reference function (tests/golden/ref_vectors_snpcall.npz), and it in turn is what the device output is compared with where
no reference output exists (synthetic tracks).  Also the comparison rule of the ninth column, shared by the CPU and the GPU tests."""
import math
import re

import numpy as np

F = np.float32

# ---- tolerances of the p-value comparison |p - p_ref| <= rel * p_ref + floor -------------------------------------------------------
# MEASURED by tests/golden/make_snp_call_fixtures.py (it prints them), not chosen: the largest relative difference (where p_ref > 1e-9)
# and the largest absolute difference between this restatement (closed forms, glibc) and the unmodified reference function with GSL 1.9
# over the vectors of ref_vectors_snpcall.npz, each TIMES TWO for the device's pow / log / erf (another libm, a few ulp).
MEASURED_REL = 1.14e-13       # largest relative difference seen, p_ref > 1e-9
MEASURED_ABS = 3.11e-15       # largest absolute difference seen
P_REL = 2 * MEASURED_REL
P_FLOOR = 2 * MEASURED_ABS
# text against text ("%.2e"): one unit in the last printed digit
TEXT_REL = 1e-2
# driver against the reference program: the deposited sums differ by fp32 atomic order (compare_tracks allows 1e-4 relative + 2e-5);
# MEASURED: the largest relative change of the p-value when every sum of a row of tests/golden/ref_runs_snp/ is moved to either end of
# that interval (all 32 combinations), over the rows with p_ref > P_FLOOR; plus the 1e-2 of the printing
MEASURED_TRACK_REL = 1.63e-2
RUN_REL = MEASURED_TRACK_REL + TEXT_REL
# rows that may be left out of the letter comparison: at most this share of the rows that carry a call
MAX_SKIPPED_SHARE = 0.005


def max_pos(c):
    m = 0
    for i in range(1, 5):
        if c[m] < c[i]:
            m = i
    return m


def _term(c, arg):
    return 0.0 if c == 0.0 else c * math.log(arg)


def _log_ratio1(c1, s):
    return s * math.log(.2) - (_term(c1, c1 / s if s else float("nan")) + _term(s - c1, ((s - c1) / s) / 4 if s else float("nan")))


def _pval(lr, df):
    x = -2 * lr
    if not x > 0.0:
        return 1.0
    P = math.erf(math.sqrt(x / 2)) if df == 1 else 1.0 - math.exp(-x / 2)
    return 1 - P


def _fdiv(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return F(a) / F(b)


def is_snp(counts, monop=False, detail=False):
    """(p, pos1, pos2, dip); pos2 = -1 where there is no second allele.  detail=True appends (pval1, pval2, ratio) of the diploid test
    (pval2 None in the forced case): what the comparison rule needs to recognise a row that sits on a decision point."""
    c = [F(x) for x in counts]
    p1 = max_pos(c)
    if monop:
        fs = F(F(F(F(c[0] + c[1]) + c[2]) + c[3]) + c[4])
        p = _pval(_log_ratio1(float(c[p1]), float(fs)), 1)
        return (p, p1, -1, False, p, None, None) if detail else (p, p1, -1, False)
    s = 0.0
    for x in c:
        s += float(x)
    pval1 = _pval(_log_ratio1(float(c[p1]), s), 1)
    second = list(c); second[p1] = F(0)
    p2 = max_pos(second)
    ratio = _fdiv(c[p1], c[p2])
    if ratio > F(3.0) or p1 == p2:
        return (pval1, p1, -1, False, pval1, None, float(ratio)) if detail else (pval1, p1, -1, False)
    for i in range(5):
        c[i] = F(float(c[i]) + 0.2); s += 0.2
    c1, c2 = float(c[p1]), float(c[p2])
    lr1 = _log_ratio1(c1, s)
    pval1 = _pval(lr1, 1)
    lr2 = s * math.log(.2) - (_term(c1, c1 / s) + _term(c2, c2 / s) + _term(s - c1 - c2, ((s - c1 + c2) / s) / 3))
    pval2 = _pval(lr2, 2)
    for i in range(5):
        c[i] = F(float(c[i]) - 0.2)
    ratio = _fdiv(c[p1], c[p2])
    near = bool(ratio < F(3.0))
    if pval2 == 0 and pval1 == 0:
        out = (0.0, p1, p2, lr2 < lr1 and near)
    elif pval2 < pval1 and near:
        out = (pval2, p1, p2, True)
    else:
        out = (pval1, p1, p2, False)
    return out + (pval1, pval2, float(ratio)) if detail else out


def call_text(counts, ref_base, pval_cut, monop):
    """the ninth column PrintSNPCall prints for a row (ref_base 0..3, pval_cut the FLOAT cutoff)"""
    p, p1, p2, dip = is_snp(counts, monop)
    if p1 == ref_base and not dip:
        return "N"
    yn = "Y" if p < float(F(pval_cut)) else "N"
    alt = "acgtn"[p1] + ("/" + "acgtn"[p2] if dip else "")
    return "%s:%s->%s p_val=%.2e" % (yn, "acgt"[ref_base], alt, p)


CALL_RE = re.compile(r"^([YN]):([acgt])->([acgtn])(?:/([acgtn]))? p_val=(\S+)$")


def parse_call(text):
    """ninth column -> None for 'N', else (letters, p): letters = everything but the digits of the p-value"""
    if text == "N":
        return None
    m = CALL_RE.match(text)
    assert m, text
    return (m.group(1), m.group(2), m.group(3), m.group(4)), float(m.group(5))


def p_close(p, p_ref, rel, floor=P_FLOOR):
    return abs(p - p_ref) <= rel * p_ref + floor


def on_decision_point(counts, p_ref, pval_cut, monop, rel, floor=P_FLOOR, ratio_rel=2.0 ** -23):
    """the reference p-value (or one of the two p-values dipLRT chooses between) lies within the comparison band of a decision point:
    the cutoff, pval1 against pval2, both p-values in the cancellation zone (the `== 0` branch), the 3.0 ratio within one float ulp
    (ratio_rel: wider where the counts themselves carry an allowance)"""
    band = lambda a, b: abs(a - b) <= rel * max(abs(a), abs(b)) + floor
    if band(p_ref, float(F(pval_cut))):
        return True
    if monop:
        return False
    _, _, _, _, pv1, pv2, ratio = is_snp(counts, False, detail=True)
    if ratio is not None and math.isfinite(ratio) and abs(ratio - 3.0) <= 3.0 * ratio_rel:
        return True
    if pv2 is None:
        return False
    return band(pv1, pv2) or (pv1 <= floor and pv2 <= floor)
