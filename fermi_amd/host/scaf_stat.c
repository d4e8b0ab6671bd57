/* scaf_stat.c -- what `scaf` (scaf_cmd.c) needs from numerics, host only: a local alignment WITH coordinates for the overlap of two unitig ends
 * (the reference's ksw_align with KSW_XSTART, scaf.c:504) and the statistics behind the P-value of a gap (scaf.c:290-335, :371-378).
 *
 * The alignment.  Match +1, mismatch -3, a gap of k bases 5 + 2k, codes 0..4 (a code above 4 matches nothing).  The reference runs the striped
 * 16-bit kernel (ksw.c:223-321) twice: forward for the score and both ends, then over the two reversed prefixes for the starts.  Its cell values
 * are those of the plain recurrence below (a gap that opens right after a gap in the other sequence is never cheaper than mismatches at these
 * costs, so the kernel's one shortcut changes no cell); what has to be told the kernel's way is which of several equal cells it reports:
 *   - the target end is the FIRST row whose best cell exceeds every earlier row's;
 *   - the query end is, among the best cells of that row, the first in the kernel's memory order: the query is cut into 8 stripes of
 *     slen = ceil(qlen / 8) positions, and position p sits at p % slen * 8 + p / slen.  The stripes are padded with positions that score 0
 *     against everything; they are part of the row and are carried here too.
 *   - the second pass stops at the first row that reaches the forward score; the starts are valid only if it reaches exactly that score. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "scaf.h"

#define SA_MATCH 1
#define SA_MISMATCH (-3)
#define SA_GAP_FIRST 7
#define SA_GAP_EXT 2

/* one pass: score, first row that reaches it (-1: none), query end by the kernel's order.  stop_at < 0: no early stop */
static int sa_pass(int ql, const uint8_t *q, int tl, const uint8_t *t, int stop_at, int *score, int *te, int *qe)
{
    const int slen = (ql + 7) / 8, w = slen * 8;
    int *h = (int *)calloc(3 * (size_t)(w > 0 ? w : 1), sizeof(int)), *e, *best, i, j, gmax = 0, row = -1;
    if (!h) return -1;
    e = h + w; best = e + w;
    for (i = 0; i < tl; ++i) {
        const int c = t[i];
        int diag = 0, f = 0, imax = 0;
        for (j = 0; j < w; ++j) {
            int x = diag + (j >= ql ? 0 : (c == q[j] && c < 5 ? SA_MATCH : SA_MISMATCH)), g;
            if (x < e[j]) x = e[j];
            if (x < f) x = f;
            diag = h[j]; h[j] = x;
            if (x > imax) imax = x;
            g = x - SA_GAP_FIRST; if (g < 0) g = 0;
            e[j] -= SA_GAP_EXT; if (e[j] < g) e[j] = g;
            f -= SA_GAP_EXT; if (f < g) f = g;
        }
        if (imax > gmax) {
            gmax = imax; row = i;
            memcpy(best, h, (size_t)w * sizeof(int));
            if (stop_at >= 0 && gmax >= stop_at) break;
        }
    }
    *score = gmax; *te = row; *qe = -1;
    for (i = 0, j = -1; i < w; ++i) {                      /* memory order: stripe position first, stripe second */
        const int p = i / 8 + i % 8 * slen;
        if (best[p] > j) { j = best[p]; *qe = p; }
    }
    free(h);
    return 0;
}

int fmdh_sw_align(int ql, const uint8_t *q, int tl, const uint8_t *t, fmdh_swaln_t *r)
{
    uint8_t *rq, *rt;
    int i, s2, te2, qe2;
    r->score = 0; r->te = r->qe = r->tb = r->qb = -1;
    if (ql <= 0 || tl < 0) return 0;
    if (sa_pass(ql, q, tl, t, -1, &r->score, &r->te, &r->qe)) return -1;
    /* the reversed prefixes; the target keeps what follows its prefix (the reference reverses in place and passes the whole length) */
    rq = (uint8_t *)malloc((size_t)r->qe + 2); rt = (uint8_t *)malloc((size_t)tl + 1);
    if (!rq || !rt) { free(rq); free(rt); return -1; }
    for (i = 0; i <= r->qe; ++i) rq[i] = q[r->qe - i];
    for (i = 0; i <= r->te; ++i) rt[i] = t[r->te - i];
    for (i = r->te + 1; i < tl; ++i) rt[i] = t[i];
    i = sa_pass(r->qe + 1, rq, tl, rt, r->score, &s2, &te2, &qe2);
    free(rq); free(rt);
    if (i) return -1;
    if (s2 == r->score) { r->tb = r->te - te2; r->qb = r->qe - qe2; }
    return 0;
}

/* ---- log-gamma (Lanczos, g = 7 with eight terms, summed from the last term to the first) and the regularised incomplete beta function by
 * the modified Lentz evaluation of its continued fraction: every operation in double and in this order, because the P-value is printed
 * with two digits and compared with thresholds ---- */
double fmdh_kf_lgamma(double z)
{
    static const double c[8] = {676.5203681218835, -1259.139216722289, 771.3234287757674, -176.6150291498386, 12.50734324009056, -0.1385710331296526,
                                0.9934937113930748e-05, 0.1659470187408462e-06};
    double x = 0;
    int i;
    for (i = 7; i >= 1; --i) x += c[i] / (z + i);
    x += c[0] / z;
    x += 0.9999999999995183;
    return log(x) - 5.58106146679532777 - z + (z - 0.5) * log(z + 6.5);
}

/* the continued fraction of I_x(a, b), modified Lentz: term j of the fraction, then the two running ratios, each kept away from zero */
static inline double cf_term(double a, double b, double x, int j)
{
    const int m = j >> 1;
    return (j & 1) ? -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1)) : m * (b - m) * x / ((a + 2 * m - 1) * (a + 2 * m));
}
static inline double not_below(double v, double floor_) { return v < floor_ ? floor_ : v; }
static double betai_fraction(double a, double b, double x)
{
    const double tiny = 1e-290, close_enough = 1e-14;
    double up = 1., down = 0., product = 1., log_front;
    int j;
    if (x == 0. || x == 1.) return x;
    for (j = 1; j < 200; ++j) {
        const double term = cf_term(a, b, x, j);
        double step;
        down = 1. / not_below(1. + term * down, tiny);
        up = not_below(1. + term / up, tiny);
        step = up * down;
        product *= step;
        if (fabs(step - 1.) < close_enough) break;
    }
    log_front = fmdh_kf_lgamma(a + b) - fmdh_kf_lgamma(a) - fmdh_kf_lgamma(b) + a * log(x) + b * log(1. - x);
    return exp(log_front) / a / product;
}
double fmdh_kf_betai(double a, double b, double x)
{
    return x < (a + 1.) / (a + b + 2.) ? betai_fraction(a, b, x) : 1. - betai_fraction(b, a, 1. - x);
}

/* the mean insert size among the pairs that can span a gap at all: those longer than l (scaf.c:371-378) */
double fmdh_scaf_correct_mean(double l, double mu, double sigma)
{
    const double x = (l - mu) / sigma, y = M_SQRT2 / M_2_SQRTPI * erfc(x * M_SQRT1_2), z = exp(-.5 * x * x);
    return mu + sigma * y / (z - x * y);
}

/* Student's t of n >= 2 pair distances (their sum and sum of squares) against mu, as the two-sided P-value scaf prints (scaf.c:400-405) */
double fmdh_scaf_pvalue(int n, int64_t sum, int64_t sum2, double mu)
{
    const double avg = (double)sum / n;
    double t = sqrt(((double)sum2 / n - avg * avg) / (n - 1));
    t = (avg - mu) / t;
    --n;
    if (n > 50) n = 50;
    return fmdh_kf_betai(.5 * n, .5, n / (n + t * t));
}
