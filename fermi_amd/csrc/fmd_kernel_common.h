// fmd_kernel_common.h -- small device helpers shared by the search kernels (overlap, SMEM, k-mer harvest)
#pragma once
#include "fmd_internal.h"

#define NONE64 (~0ull)
#define FMD_SZ_MASK 0xffffffffffffull

__device__ __forceinline__ int comp6(int c) { return (c >= 1 && c <= 4) ? 5 - c : c; }

#include "fmd_search.h"   // the read window, the prefix-table start and the result triple of the backward-search kernels

template <class T>
__device__ __forceinline__ T sel6(int c, T a0, T a1, T a2, T a3, T a4, T a5)
{
    T r = a0;
    r = c == 1 ? a1 : r; r = c == 2 ? a2 : r; r = c == 3 ? a3 : r; r = c == 4 ? a4 : r; r = c == 5 ? a5 : r;
    return r;
}

__device__ __forceinline__ void load_entry(const fmd_intv_t *e, uint64_t &x0, uint64_t &x1, uint64_t &sz, uint64_t &info)
{
    const uint4 *q = (const uint4 *)e;
    const uint4 a = q[0], b = q[1];
    x0 = (uint64_t)a.y << 32 | a.x; x1 = (uint64_t)a.w << 32 | a.z;
    sz = (uint64_t)b.y << 32 | b.x; info = (uint64_t)b.w << 32 | b.z;
}
__device__ __forceinline__ void store_entry(fmd_intv_t *e, uint64_t x0, uint64_t x1, uint64_t sz, uint64_t info)
{
    uint4 *q = (uint4 *)e;
    q[0] = make_uint4((uint32_t)x0, (uint32_t)(x0 >> 32), (uint32_t)x1, (uint32_t)(x1 >> 32));
    q[1] = make_uint4((uint32_t)sz, (uint32_t)(sz >> 32), (uint32_t)info, (uint32_t)(info >> 32));
}

// Candidate intervals of one strand (the list overlap_intv builds, unitig.c:38-64), as the walk leaves them for the get_nei kernels.
// Wide form = store_entry(x0, x1, size, depth).  Narrow form (size <= 63, depth < 65536: every candidate the walk pushes from its
// 64-position window path) carries two more facts about BWT[x0, x0 + size) that the walk has at hand when it pushes and that
// fm6_get_nei would otherwise fetch the block of x0 for again: D = the positions of '$' in that range (bit i = BWT[x0 + i] is '$':
// the reads that START with the candidate string, the sentinel tests of unitig.c:112/:129) and r0 = the number of '$' before x0
// (x[0] of the neighbour interval, unitig.c:113).  Both follow a forward extension without touching memory (the child ranges are
// sub-ranges of [x0, x0 + size)), so the unforked fast path of get_nei (k_ovl_nei_fast) never reads the x[0] side at all.
//   q[0] = { x0 lo, x0 bits 32..39 | r0 bits 32..39 << 8 | depth << 16, x1 lo, x1 hi }     q[1] = { D lo, D hi, r0 lo, NARROW | size }
#define FMD_CAND_NARROW 0x80000000u
struct FmdCand { uint64_t x0, x1, sz, D, r0; uint32_t depth; bool narrow; };
__device__ __forceinline__ FmdCand cand_decode(const uint4 a, const uint4 b)
{
    FmdCand c;
    c.narrow = (b.w & FMD_CAND_NARROW) != 0;
    c.x1 = (uint64_t)a.w << 32 | a.z;
    if (c.narrow) {
        c.x0 = (uint64_t)(a.y & 0xffu) << 32 | a.x; c.r0 = (uint64_t)((a.y >> 8) & 0xffu) << 32 | b.z; c.depth = a.y >> 16;
        c.sz = b.w & 63u; c.D = (uint64_t)b.y << 32 | b.x;
    } else {
        c.x0 = (uint64_t)a.y << 32 | a.x; c.sz = ((uint64_t)b.y << 32 | b.x) & 0xffffffffffffull; c.depth = b.z; c.D = 0; c.r0 = 0;
    }
    return c;
}
// (one candidate in either form: the words are chosen first and leave in two 16-byte stores -- a store_entry and a narrow store under an if compile to three)
__device__ __forceinline__ void cand_store(fmd_intv_t *e, bool narrow, uint64_t x0, uint64_t x1, uint64_t sz, uint32_t depth, uint64_t D, uint64_t r0)
{
    uint4 *q = (uint4 *)e;
    const uint32_t x0h = (uint32_t)(x0 >> 32);
    q[0] = make_uint4((uint32_t)x0, narrow ? ((x0h & 0xffu) | ((uint32_t)(r0 >> 32) & 0xffu) << 8 | depth << 16) : x0h, (uint32_t)x1, (uint32_t)(x1 >> 32));
    q[1] = make_uint4(narrow ? (uint32_t)D : (uint32_t)sz, narrow ? (uint32_t)(D >> 32) : (uint32_t)(sz >> 32), narrow ? (uint32_t)r0 : depth,
                      narrow ? (FMD_CAND_NARROW | (uint32_t)sz) : 0u);
}

// ---- 64-position window over a lane's block images (used when an SA interval is narrower than 64)
__device__ __forceinline__ uint64_t bits_below(int j) { return j >= 64 ? ~0ull : ((1ull << j) - 1); }

// The three 32-position chunks (bit-plane words) that cover BWT[pos, pos + 64), from the lane's block
// images: img_k holds block blk_k (when has_k), img_l holds blk_l (when has_l).  Words of other blocks
// read as zero (they are masked out by the callers' range masks).
__device__ __forceinline__ uint4 grp_pick(const uint4 *img_k, int t_k, const uint4 *img_l, int t_l, uint32_t blk_k, uint32_t blk_l,
                                          bool has_k, bool has_l, uint32_t blk, uint32_t ch)
{
    const bool in_k = has_k && blk == blk_k, in_l = has_l && blk == blk_l;
    uint4 v = in_k ? img_k[(int)ch ^ t_k] : img_l[(int)ch ^ t_l];
    if (!in_k && !in_l) v = make_uint4(0, 0, 0, 0);
    return v;
}
// The window starts one position after `p`, whose block and offset (blk_p, off_p) the caller already has
// (p = the k side of the rank pair that brought the images in): no second division.
__device__ __forceinline__ void grp_window(const uint4 *img_k, int t_k, const uint4 *img_l, int t_l, uint32_t blk_k, uint32_t blk_l,
                                           bool has_k, bool has_l, uint32_t blk_p, uint32_t off_p, uint4 &a, uint4 &b, uint4 &c)
{
    uint32_t blk = blk_p, ch = (off_p + 1) >> 5;
    // 32-position words counted from the start of block blk_p: words 0..2 are its chunks, word q >= 3 is chunk q - 2 of the next block
    if (ch >= FMD_BLK_CHUNKS) { ch -= FMD_BLK_OWN_CHUNKS; ++blk; }
    a = grp_pick(img_k, t_k, img_l, t_l, blk_k, blk_l, has_k, has_l, blk, ch);
    if (++ch == FMD_BLK_CHUNKS) { ch = FMD_BLK_CHUNKS - FMD_BLK_OWN_CHUNKS; ++blk; }
    b = grp_pick(img_k, t_k, img_l, t_l, blk_k, blk_l, has_k, has_l, blk, ch);
    if (++ch == FMD_BLK_CHUNKS) { ch = FMD_BLK_CHUNKS - FMD_BLK_OWN_CHUNKS; ++blk; }
    c = grp_pick(img_k, t_k, img_l, t_l, blk_k, blk_l, has_k, has_l, blk, ch);
}
__device__ __forceinline__ uint64_t win64(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t sh)
{
    // two funnel shifts (v_alignbit_b32: low word of {hi, lo} >> sh, sh in 0..31)
    const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh), hi = __builtin_amdgcn_alignbit(w2, w1, sh);
    return (uint64_t)hi << 32 | lo;
}
// The positions of a window (planes X, Y, Z) whose symbol sorts before c in the order of fm6_extend's x[1] sums, 0 < 4 < 3 < 2 < 1 < 5 (exact.c:81-86);
// cx, cy, cz = all ones where c has the plane's bit.  '$' sorts before every base; T (z alone) before c = 3, 2, 1, 5: c has x or y; G (x and y) before
// 2, 1, 5: exactly one of them; C (y alone) before 1, 5: x without y; A (x alone) before 5: x and z.  Without a branch on c: the lanes of a wave differ in it.
template <class T>
__device__ __forceinline__ T win_before(T X, T Y, T Z, T cx, T cy, T cz)
{
    return ~(X | Y | Z) | (Z & ~X & (cx | cy)) | (X & Y & (cx ^ cy)) | (Y & ~X & cx & ~cy) | (X & ~Y & ~Z & cx & cz);
}
__device__ __forceinline__ uint64_t range64(uint32_t a, uint32_t b) // bits [a, b), b <= 64
{
    return bits_below((int)b) & ~bits_below((int)a);
}


// Work lists of the get_nei kernels.  A strand with m candidate intervals goes to the group kernel with
// the smallest group size G >= m (one lane per candidate, 64 / G strands per wave); the sizes are chosen
// so that 64 / G groups leave at most 4 lanes unused.  G = 4 is there for reads with errors: an error cuts the overlaps a
// strand has short, and 36 % of the strands of 30-fold reads with 1 % substitutions that have any candidate have at most four
// (error-free: 0.1 %) -- in groups of 8 half of their lanes never hold anything.
#define FMD_GRP_CLASSES 6
__device__ __host__ __forceinline__ constexpr int fmd_grp_size(int k) { return k == 0 ? 4 : k == 1 ? 8 : k == 2 ? 12 : k == 3 ? 16 : k == 4 ? 21 : 32; }
// hand-over from k_ovl_nei_fast to k_ovl_nei_grp: list slots reserved FMD_FAST_CHUNK at a time, unused ones stay holes
#define FMD_FAST_CHUNK 16
#define FMD_FAST_MAX_WAVES 8192
#define FMD_LIST_HOLE 0xffffffffu
// A strand k_ovl_nei_fast hands on in the middle (a fork, an N: rounds only k_ovl_nei_grp does) travels with its state: bit 15 of the
// list entry's second word, the number of live candidates in the bits below, and in the strand's row of listB (scratch of
// k_ovl_nei, which these strands never reach without being started over from listA) one 32-byte entry per live candidate, in list
// order.  Every entry also carries the strand's own state (round, neighbours so far, lfork, info of the first neighbour): the lanes
// of a group read one entry each and nothing else.
//   a = { x1 lo, x1 bits 32..39 | round << 8 | n_nei << 24, D lo, D hi }     b = { r0 lo, r0 bits 32..39 | nei0 << 8, size | pos << 16, lfork (17 bits) | category << 17 | flags << 22 }
// (category, flags: a strand k_ovl_nei_grp<G> passes on to a larger group size because a round leaves it more than G candidates)
#define FMD_LIST_RESUME 0x8000u
__device__ __forceinline__ void fmd_resume_encode(uint4 *e, uint64_t x1, uint32_t sz, uint64_t D, uint64_t r0, uint32_t pos, uint32_t round, uint32_t n_nei, uint32_t nei0, uint32_t lf,
                                                  uint32_t cat = 0, uint32_t flags8 = 0)
{
    e[0] = make_uint4((uint32_t)x1, ((uint32_t)(x1 >> 32) & 0xffu) | round << 8 | n_nei << 24, (uint32_t)D, (uint32_t)(D >> 32));
    e[1] = make_uint4((uint32_t)r0, ((uint32_t)(r0 >> 32) & 0xffu) | nei0 << 8, sz | pos << 16, (lf & 0x1ffffu) | cat << 17 | (flags8 & 0xffu) << 22);
}
__device__ __forceinline__ bool fmd_resume_fits(uint32_t round, uint32_t n_nei, uint32_t nei0, uint32_t pos) { return round < 65536u && n_nei < 256u && nei0 < 65536u && pos < 65536u; }
__device__ __forceinline__ void fmd_resume_decode(const uint4 a, const uint4 b, uint64_t &x1, uint32_t &sz, uint64_t &D, uint64_t &r0, uint32_t &pos, uint32_t &round, uint32_t &n_nei,
                                                  uint32_t &nei0, uint32_t &lf, uint32_t &cat, uint32_t &flags8)
{
    x1 = (uint64_t)(a.y & 0xffu) << 32 | a.x; round = (a.y >> 8) & 0xffffu; n_nei = a.y >> 24; D = (uint64_t)a.w << 32 | a.z;
    r0 = (uint64_t)(b.y & 0xffu) << 32 | b.x; nei0 = b.y >> 8; sz = b.z & 0xffffu; pos = b.z >> 16; lf = b.w & 0x1ffffu; cat = (b.w >> 17) & 31u; flags8 = (b.w >> 22) & 0xffu;
}
#define FMD_LANE_CHUNK 64                  // the same for k_ovl_nei_lane (fmd_ovlp_lane.hip): every lane of a wave may hand its strand on in one step
#define FMD_FAST_RESERVE (2 * FMD_FAST_MAX_WAVES * FMD_LANE_CHUNK)   // entries a general list may lose to holes (two fast kernels feed it; a wave's last chunk keeps at most FMD_LANE_CHUNK - 1)

// ---- The work lists of ONE PART of a batch (np strands), laid over a uint32_t area: FMD_CLS_HEADER_U32 words of counters -- one 128-byte line per list --, then
// the lists.  This is the only place that knows where they lie: the host fills FmdOvlClasses through fmd_cls_list (fmd_nei_lists_at, fmd_ovlp_internal.h), the
// walk's close finds its list through it.  List numbers: general class k = k, the slow list = FMD_CLS_SLOW, fast class k = fmd_cls_fast(k) with 32-bit masks
// and fmd_cls_fast(k + FMD_GRP_CLASSES) with 64-bit masks.
//   general list k   2 words per entry (slot of the batch, candidates | length << 16); room for every strand of the part + FMD_FAST_RESERVE holes
//   the slow list    1 word per entry, np entries: what classification sets aside (k_ovl_nei takes them at once, beside the group kernels)
//   fast list k      2 words per entry, np entries; when the fast kernels are through, the storage of the SECOND-PASS list of class k (k_ovl_nei_grp)
//   the late list    1 word per entry, np entries: strands the fast / group kernels hand back (a second k_ovl_nei launch behind them)
//   the fix-up list  1 word per entry, np entries: strands a group kernel closed with one neighbour after a fork (k_ovl_fix)
#define FMD_CLS_CNT_STRIDE 32                                   // counters sit on separate 128-byte lines
#define FMD_CLS_HEADER_U32 640                                  // the counter area in front of the lists
#define FMD_CLS_LISTS (3 * FMD_GRP_CLASSES + 1)                 // general lists, the slow list, fast lists (32-bit masks, 64-bit masks): the lists that have a counter line
#define FMD_CLS_SLOW FMD_GRP_CLASSES
static_assert(FMD_CLS_LISTS * FMD_CLS_CNT_STRIDE <= FMD_CLS_HEADER_U32, "one counter line per list");
__host__ __device__ __forceinline__ constexpr int fmd_cls_fast(int k) { return FMD_GRP_CLASSES + 1 + k; }     // k in [0, 2 * FMD_GRP_CLASSES)
__host__ __device__ __forceinline__ constexpr int fmd_cls_cnt_off(int c) { return c * FMD_CLS_CNT_STRIDE; }    // word offset of the counter line of list c
// List c of a part of np strands, c in [0, FMD_CLS_LISTS]: as a pointer (P = uint32_t *, area = the part's), or as a word offset (P = size_t, area = 0).
// In this shape -- the slow list first, then a select between two pointers -- it folds into k_ovl_walk<WALK_TAIL2> without a register (that kernel has none
// to give: 125 of 128); as `area + offset(c)` it cost two.
template <class P>
__host__ __device__ __forceinline__ constexpr P fmd_cls_list(P area, int c, size_t np)
{
    const size_t gl = 2 * np + 2 * (size_t)FMD_FAST_RESERVE;          // words of a general list
    const P slow = area + FMD_CLS_HEADER_U32 + gl * FMD_GRP_CLASSES;
    if (c == FMD_CLS_SLOW) return slow;
    return c < FMD_CLS_SLOW ? area + FMD_CLS_HEADER_U32 + gl * c : slow + np + 2 * np * (size_t)(c - FMD_CLS_SLOW - 1);
}
template <class P> __host__ __device__ __forceinline__ constexpr P fmd_cls_late(P area, size_t np) { return fmd_cls_list(area, FMD_CLS_LISTS, np); }   // behind the last fast list
template <class P> __host__ __device__ __forceinline__ constexpr P fmd_cls_fix(P area, size_t np) { return fmd_cls_late(area, np) + np; }
// A batch cut into parts (FMD_OVLP_PIPE) keeps one such area per part, one behind the other: per part a header and the general lists' reserve, per strand
// the words that grow with the part.  The area of part `part`, whose first strand is strand b of the batch, starts at word
#define FMD_CLS_WORDS_PER_STRAND (6 * FMD_GRP_CLASSES + 3)      // two words per entry of a general and of a fast list, one each for the slow, the late and the fix-up list
#define FMD_CLS_PART_U32 (FMD_CLS_HEADER_U32 + 2 * FMD_GRP_CLASSES * FMD_FAST_RESERVE)
__host__ __device__ __forceinline__ constexpr size_t fmd_cls_part_off(int part, size_t b) { return (size_t)part * FMD_CLS_PART_U32 + b * FMD_CLS_WORDS_PER_STRAND; }
static_assert(fmd_cls_fix<size_t>(0, 1000) + 1000 == fmd_cls_part_off(1, 1000) && fmd_cls_fix<size_t>(0, 1) + 1 == fmd_cls_part_off(1, 1), "a part's lists end where the next part begins");

// The words of a counter line (zeroed with the header before every batch).  Kernels get a pointer to ONE word of a line -- the count of the list they read,
// the count they append to -- and reach its neighbours by the difference of two names.
enum FmdClsWord {
    // every line
    FMD_CW_COUNT = 0,            // entries of the list (a general list: slots, the holes of the chunked hand-over included)
    // a general and a fast list's line
    FMD_CW_DEAL = 16,            // the next position to deal out: fmd_deal_next of the group kernels, the ticket counter of k_ovl_nei_lane
    // a fast list's line
    FMD_CW_DOWN = 4,             // entries of the second-pass list of the class (strands k_ovl_nei_grp moved to a smaller group), in chunks of FMD_FAST_CHUNK
    FMD_CW_DOWN_DEAL = FMD_CW_DOWN + FMD_CW_DEAL,   // ... and the deal counter of that list: the second pass is launched with FMD_CW_DOWN as its count
    FMD_CW_HANDED = 8,           // strands the fast kernel handed on to the general list of the class (`bail_n`; FMD_OVLP_STATS)
    FMD_CW_HANDED_AT0 = 9,       // (printed by the GRP_STATS block; nothing counts here since strands are handed on where they stand)
    FMD_CW_FAST_ROUNDS = 10,     // GRP_STATS, the fast kernels: wave rounds,
    FMD_CW_FAST_LIVE = 11,       // ... live lanes in them,
    FMD_CW_FAST_HELD = 12,       // ... lanes of groups that hold a strand,
    FMD_CW_FAST_ROUNDS2 = 13,    // ... rounds in which some strand saw a second base
    FMD_CW_LANE_ADM = 21,        // FMD_OVLP_STATS, k_ovl_nei_lane's counting instantiations (six words, in LaneStats' order): strands admitted,
    FMD_CW_LANE_QUIET = 22,      // ... lane rounds: quiet,
    FMD_CW_LANE_SELF = 23,       // ... the self-end round inline,
    FMD_CW_LANE_CLOSE = 24,      // ... the closing round inline,
    FMD_CW_LANE_FULL = 25,       // ... through the full round code,
    FMD_CW_LANE_MAT = 26,        // ... of those, with a pending self-end round to apply to the column first
    // the slow list's line
    FMD_CW_LATE = 4,             // entries of the late list (`slow_n` of the fast / group kernels)
    FMD_CW_GRP_ROUNDS = 12,      // GRP_STATS, the group kernels: wave rounds,
    FMD_CW_GRP_LIVE = 13,        // ... live lanes in them,
    FMD_CW_GRP_HELD = 14,        // ... lanes of groups that hold a strand
    FMD_CW_FIX = 20,             // entries of the fix-up list
};
template <int... W> constexpr bool fmd_cw_distinct()
{
    const int w[] = {W...};
    for (size_t i = 0; i < sizeof...(W); ++i) {
        if (w[i] < 0 || w[i] >= FMD_CLS_CNT_STRIDE) return false;
        for (size_t j = 0; j < i; ++j) if (w[j] == w[i]) return false;
    }
    return true;
}
static_assert(fmd_cw_distinct<FMD_CW_COUNT, FMD_CW_DEAL>(), "a general list's counter line");
static_assert(fmd_cw_distinct<FMD_CW_COUNT, FMD_CW_DEAL, FMD_CW_DOWN, FMD_CW_DOWN_DEAL, FMD_CW_HANDED, FMD_CW_HANDED_AT0, FMD_CW_FAST_ROUNDS, FMD_CW_FAST_LIVE, FMD_CW_FAST_HELD,
                              FMD_CW_FAST_ROUNDS2, FMD_CW_LANE_ADM, FMD_CW_LANE_QUIET, FMD_CW_LANE_SELF, FMD_CW_LANE_CLOSE, FMD_CW_LANE_FULL, FMD_CW_LANE_MAT>(), "a fast list's counter line");
static_assert(fmd_cw_distinct<FMD_CW_COUNT, FMD_CW_LATE, FMD_CW_GRP_ROUNDS, FMD_CW_GRP_LIVE, FMD_CW_GRP_HELD, FMD_CW_FIX>(), "the slow list's counter line");

// The lists of one part as pointers (the kernels' form; filled through the functions above).  The late and the fix-up list travel beside it (NeiArgs,
// fmd_ovlp_internal.h): the kernels that append to them get them as `slow_list` and `fix_off`.
struct FmdOvlClasses {
    uint32_t *cnt;                        // the header: line fmd_cls_cnt_off(c) belongs to list c, words FmdClsWord
    uint32_t *lst[FMD_GRP_CLASSES];       // the general lists
    uint32_t *lslow;                      // the slow list
    uint32_t *fast[2 * FMD_GRP_CLASSES];  // strands whose candidates are in the narrow form: k_ovl_nei_fast / k_ovl_nei_lane first; [FMD_GRP_CLASSES ..]: the 64-bit lists
};

// The list a strand belongs on, from what is known of it at the walk's close (k_ovl_walk<WALK_TAIL2>) or from its record and its row of listA (k_ovl_classify):
// m candidates, len bases, and three facts about the WIDEST candidate -- the first one pushed, the last of the list (shortest overlap): its size is at most
// 63 (the group kernels count symbols of BWT[x, x + size) through a 64-position window), it is in the narrow form (the fast kernels check the others when
// they load them), its size is more than 31 (the fast kernels' 64-bit masks).  A strand goes to the smallest group class >= min_cls that holds its m
// candidates, to that class's fast list where use_fast; everything else to the slow list.  Who is eligible at all (status 0, candidates, no overflow, not
// contained) is the caller's test: the two read it from different places.
__device__ __forceinline__ int fmd_ovl_list_of(uint32_t m, uint32_t len, bool w63, bool wnarrow, bool w32, int use_fast, int min_cls)
{
    int c = FMD_CLS_SLOW;
    if (w63 && len < 65535u) {
#pragma unroll
        for (int k = FMD_GRP_CLASSES - 1; k >= 0; --k) if (k >= min_cls && m <= (uint32_t)fmd_grp_size(k)) c = k;
        if (c < FMD_CLS_SLOW && wnarrow && use_fast) c += fmd_cls_fast(w32 ? FMD_GRP_CLASSES : 0);   // fast list c, or c + FMD_GRP_CLASSES
    }
    return c;
}

// Two-pass walk of a sorted job (k_ovl_walk<WALK_HEAD / WALK_TAIL>, fmd_ovlp_walk.hip): where a strand stands FMD_WALK_SPLIT bases in.
#define FMD_WALK_SPLIT 32u            // a multiple of 16: the stash of a parked strand is two whole 16-byte groups
struct FmdWalkPark {                  // k = ~0: the sequence ended inside the head (its record was written there)
    unsigned long long k, x0, x1, sz;  // LF row and bi-interval after FMD_WALK_SPLIT bases
    uint4 bases;                       // those bases, last base of the sequence first, 4 bits each (nt6 codes)
    uint4 pad;                         // (the row is one 64-byte line, written in one burst)
};
static_assert(sizeof(FmdWalkPark) == 64, "one line per parked strand");
