/* swscore.c -- the one number the bubble poppers (mag_bubble.c) need from a local alignment: its score.
 * Smith-Waterman with affine gaps over three rows: H (best score of an alignment ending in the cell), E (ending in a gap in a),
 * and F carried along the row.  Match +5, mismatch -4, a gap of k bases 5 + 2k.  The reference computes this in saturating
 * 16-bit lanes (ksw.c:223-321), so no score exceeds 32767: two identical sequences of 6553 bases score 32765, of 6554 and more 32767. */
#include <stdlib.h>
#include "mag.h"

#define SW_MATCH 5
#define SW_MISMATCH (-4)
#define SW_GAP_OPEN_EXT 7      /* the first base of a gap */
#define SW_GAP_EXT 2
#define SW_MAX 32767

int fmdh_sw_score(int la, const uint8_t *a, int lb, const uint8_t *b)
{
    int stack_row[2 * 512], *h, *e, i, j, best = 0;
    if (la <= 0 || lb <= 0) return 0;
    if (la < lb) { const uint8_t *t = a; const int l = la; a = b; la = lb; b = t; lb = l; }   /* the rows follow the shorter one */
    h = lb <= 512 ? stack_row : (int *)malloc(2 * (size_t)lb * sizeof(int));
    if (!h) return -1;
    e = h + lb;
    for (j = 0; j < lb; ++j) h[j] = e[j] = 0;
    for (i = 0; i < la; ++i) {
        const uint8_t c = a[i];
        int diag = 0, f = 0;
        for (j = 0; j < lb; ++j) {
            int x = diag + (c == b[j] && c < 4 ? SW_MATCH : SW_MISMATCH), t;
            if (x > SW_MAX) x = SW_MAX;
            if (x < e[j]) x = e[j];
            if (x < f) x = f;                      /* e, f >= 0: so is x */
            diag = h[j]; h[j] = x;
            if (x > best) best = x;
            t = x - SW_GAP_OPEN_EXT;
            e[j] -= SW_GAP_EXT; if (e[j] < t) e[j] = t; if (e[j] < 0) e[j] = 0;
            f -= SW_GAP_EXT; if (f < t) f = t; if (f < 0) f = 0;
        }
    }
    if (h != stack_row) free(h);
    return best;
}
