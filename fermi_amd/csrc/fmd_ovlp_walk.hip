// fmd_ovlp_walk.hip -- overlap discovery, the walk family: the fused LF-walk + overlap_intv (k_ovl_walk in its four modes), the two-base pass
// beside it (k_ovl_pair), the kernels that feed it and tidy up behind it, and their launchers (fmd_ovlp_internal.h).
#include <stdlib.h>
#include "fmd_ovlp_internal.h"

// ------------------------------------------------- phases 0+A fused: LF-walk + overlap_intv in one pass
// fm_retrieve walks the rows k_i of the suffixes "last i bases $" of the sequence; overlap_intv
// extends the interval I_i of "last i bases" backward.  k_i lies INSIDE I_i, so once I_i is
// narrower than a rank block the LF step and the extension read the SAME block: one gather per
// base instead of two (while I_i is still wide -- the first ~log4(n) bases, blocks that live in
// L2 -- the LF step takes a gather of its own).  The base found by the LF step is the base the
// extension needs; when it is '$' the same ranks are fm6_is_contained's left test (unitig.c:83-85).
// Candidates are pushed with info = depth (their start is len - depth, known only at the end).
#ifndef FMD_HEAD_AUX
#define FMD_HEAD_AUX 0
#endif
enum { WK_IDLE = 0, WK_LF, WK_EXT, WK_BOTH, WK_RIGHT, WK_ADM1, WK_ADM2, WK_WAIT, WK_DONE };   // (WK_WAIT, WK_DONE: WALK_TAIL2 only)
// WALK_TAIL2 in phase: a lane in WK_ADM2 carries six bits of its sort key above the state (the minimizer's offset, and 32 = the key has a minimizer)
#define WK_KEY_SHIFT 4
#define WK_STATE_MASK ((1 << WK_KEY_SHIFT) - 1)
// can the LF step at row k be read from a block the backward extension of [x0, x0 + sz) brings in anyway (the block of x0 - 1, or
// the block of its other end when that one does not reach it)?
__device__ __forceinline__ bool walk_lf_shares(uint64_t k, uint64_t x0, uint64_t sz)
{
    // k lies inside [x0, x0 + sz); a range of at most 64 positions touches two consecutive blocks at most -- those of its two ends
    if (sz <= 63) return true;
    uint32_t o;
    return fmd_in_block(k, fmd_blk_of(x0 - 1), o) || fmd_in_block(k, fmd_blk_of(x0 - 1 + sz), o);
}

// cnt[c] for a lane's own c, by selects over the six values the kernel holds in SGPRs: ix.cnt[c] is a load from the argument segment, one more memory access that the
// row and the interval of the next step wait for behind every gather, and whose s_waitcnt waits for every other load in flight (profiles/walk_narrow32)
__device__ __forceinline__ uint64_t walk_cnt(const FmdIndexView &ix, int c) { return sel6(c, ix.cnt[0], ix.cnt[1], ix.cnt[2], ix.cnt[3], ix.cnt[4], ix.cnt[5]); }

// every 4th base: the word moves into its place of the 16-byte group; every 16th: one store
#define WALK_STASH_WORD()                                                                                  \
    do {                                                                                                   \
        const uint32_t wq_ = (depth >> 2) & 3;                                                             \
        if (wq_ == 1) pk0 = pack; else if (wq_ == 2) pk1 = pack; else if (wq_ == 3) pk2 = pack;            \
        else {                                                                                             \
            if (depth <= stride_r) *(uint4 *)(srev + sid * (size_t)stride_r + depth - 16) = make_uint4(pk0, pk1, pk2, pack); \
            pk0 = pk1 = pk2 = 0;                                                                           \
        }                                                                                                  \
        pack = 0;                                                                                          \
    } while (0)

// one more base of the sequence (the one at position `depth` from its end).  WALK_HEAD keeps its 32 bases in the four stash registers,
// 4 bits each (FmdWalkPark::bases), and never stores
#define WALK_PUT_BASE(cc)                                                                                  \
    do {                                                                                                   \
        if (MODE == WALK_TAIL2) {   /* 2 bits per base, a word of 16 into the lane's LDS stash */          \
            pack |= (((uint32_t)(cc) - 1u) & 3u) << (2 * (depth & 15));                                    \
            if ((uint32_t)(cc) > 4u) flags |= WALK_F_HASN;                                                 \
            ++depth;                                                                                       \
            if ((depth & 15) == 0) { if (depth <= WALK_LS_BASES) walk_ls[((depth >> 4) - 1) * 64 + fmd_lane()] = pack; pack = 0; } \
        } else                                                                                             \
        if (MODE == WALK_HEAD) {                                                                           \
            const uint32_t v_ = (uint32_t)(cc) << (4 * (depth & 7)), w_ = depth >> 3;                      \
            pk0 |= w_ == 0 ? v_ : 0u; pk1 |= w_ == 1 ? v_ : 0u; pk2 |= w_ == 2 ? v_ : 0u; pack |= w_ == 3 ? v_ : 0u; \
            ++depth;                                                                                       \
        } else {                                                                                           \
            pack |= (uint32_t)(cc) << (8 * (depth & 3));                                                   \
            ++depth;                                                                                       \
            if ((depth & 3) == 0) WALK_STASH_WORD();                                                       \
        }                                                                                                  \
    } while (0)

// Two-pass form (WALK_HEAD + WALK_TAIL, the locality sort of fmd_ovlp_sorted_dev below).  Strands whose last bases lie next to each
// other on the genome visit the SAME rank blocks (the interval of "g[a, e)" holds the interval of "g[a, e + d)"), d steps apart; in
// id order they are never in flight together and every one of those visits is a DRAM miss.  WALK_HEAD takes every strand of the job
// FMD_WALK_SPLIT bases in and parks it (FmdWalkPark: row, bi-interval, the bases so far); the strands are sorted by the minimizer of
// those bases (k_ovl_park_keys), so that strands of one genomic window sit in neighbouring lanes; WALK_TAIL picks each strand up where
// it was parked, in that order.  Nothing can be pushed before min_match >= FMD_WALK_SPLIT bases, so the two passes together make
// exactly the steps of the one-pass walk and leave the same records, candidates and stash.
enum { WALK_WHOLE = 0, WALK_HEAD = 1, WALK_TAIL = 2, WALK_TAIL2 = 3 };   // (FMD_WALK_SPLIT, FmdWalkPark: fmd_kernel_common.h)

// WALK_TAIL2 = WALK_TAIL for sequences of at most WALK_LS_BASES bases, without the stash in HBM and without k_ovl_seq_out behind it: the bases wait in
// LDS, 2 bits each (code - 1; 7 words per lane: what is left of a CU's 160 KiB beside the gather's 8.25 KiB per wave at 16 waves), and a lane that
// is through its sequence writes the caller's row itself, in read order, from those words at the strand's close (walk_emit_row: ~250 instructions for
// the wave whoever takes part, where the separate kernel read 112 + wrote 100 bytes per strand and cost the step 14 ms of its 272).  A sequence that
// holds an N (2 bits do not) is put on a list and k_ovl_seq_redo writes its row afterwards from what WALK_HEAD parked.
// Two admissions.  Free-running (WalkArgs::keys == nullptr; FMD_WALK_PHASE=0: the A/B switch): a lane takes the next strand as soon as it is idle and closes
// its strand in the step after its last; reads of one length finish a wave together, so the close has company by itself.  In phase on the genome (keys
// given: the batches of fmd_ovlp_sorted_dev): the sorted order puts the strands of one minimizer into neighbouring lanes, but admitted together they
// advance in step in DEPTH, so two of them whose ends lie d positions apart ask for the same rank block d wave steps apart, and a block survives one or
// two steps of an XCD's resident waves in its L2.  A strand whose minimizer lies o bases from its end therefore starts omax - o steps late (o = the low
// five bits of its key, omax the largest of the wave's generation).  The strands of a key then stand at the same genome position in every step:
// their nested intervals ask for the same block in the same wave instruction and share its line: half the bytes fetched and a third fewer requests per
// launch.  The price: up to 16 idle steps per lane and generation, a wave takes new strands only when all its lanes are idle (a generation
// lasts as long as its longest strand: reads of one length, which is what a job of at most WALK_LS_BASES bases holds), and the lanes of a generation
// finish in up to 17 different steps and wait in WK_DONE for a close in company (top of the loop).  On the parent's narrow turn those idle steps took back
// what the shared lines gave (profiles/walk_phase: the kernel left the L2 bound and met the issue bound); with the turn in 32-bit words (below) it has the
// instructions to spare, and the two together are what ships: the launch 25 -> 21 ms, the step 202 -> 184.5 ms (profiles/walk_phase32).
// The phase start costs no register: the six bits it needs of a strand's key (offset, has a minimizer) come in through `pack`, idle between the ticket and
// WK_ADM1, ride in the spare bits of `st` for the one step to WK_ADM2 (WK_KEY_SHIFT), and the countdown of a waiting lane is `npush`.
#define WALK_LS_WORDS 7
#define WALK_LS_BASES (16 * WALK_LS_WORDS)
#define WALK_F_HASN 0x80000000u       // (in the walk's `flags` register only: never stored)
// the strand's FIRST candidate (the widest: shortest overlap) as k_ovl_classify reads it back from listA -- size <= 63, narrow form, size > 31
#define WALK_F_W63 0x40000000u
#define WALK_F_WNARROW 0x20000000u
#define WALK_F_W32 0x10000000u
// two small fields of the walk itself, kept in `flags` and not in registers of their own: the strand is left-contained or its right extension found another
// size (the record's status -3), and the base an LF step found for the extension that follows it in a gather of its own (WK_LF -> WK_EXT)
#define WALK_F_CONTAINED 0x08000000u
#define WALK_F_CPEND_SHIFT 24
#define WALK_F_CPEND (7u << WALK_F_CPEND_SHIFT)
#define WALK_F_INTERNAL 0xff000000u
struct __attribute__((packed, aligned(4))) WalkU4 { uint32_t x, y, z, w; };   // a 16-byte store at a 4-byte aligned address
// four bases, 2 bits each, first found (= LAST in read order) in the low bits -> their nt6 codes as the four bytes of a word in read order
__device__ __forceinline__ uint32_t walk_expand4(uint32_t win8)
{
    uint32_t y = (win8 | win8 << 12) & 0x000f000fu;
    y = (y | y << 6) & 0x03030303u;
    return __builtin_bswap32(y + 0x01010101u);
}
// eight bases as nibbles (nt6 codes 1..5) -> 2 bits each (code - 1) in the low 16 bits; bit 16 set when one of them is not A/C/G/T
__device__ __forceinline__ uint32_t walk_nib_to_2bit(uint32_t v)
{
    const uint32_t t = v - 0x11111111u;
    uint32_t x = t & 0x33333333u;
    x = (x | x >> 2) & 0x0f0f0f0fu; x = (x | x >> 4) & 0x00ff00ffu; x = (x | x >> 8) & 0x0000ffffu;
    return x | ((t & 0xccccccccu) ? 0x10000u : 0u);
}
// st[w * 64]: word w of this lane (bases 16w .. 16w + 15 in the order found, i.e. from the sequence's end); len <= WALK_LS_BASES; dst 4-byte aligned
// with room for len + 3 bytes.  Output word w holds the bases found as [len - 4 - 4w, len - 4w): with r = len & 3 the words line up with the stash
// shifted by r bases, 16 bases = four output words = one 16-byte store.  The word that holds the sequence's last bases (r of them) is padded with
// zeros, bytes beyond it are not written (as k_ovl_seq_out leaves a row).
__device__ __forceinline__ void walk_emit_row(const uint32_t *st, uint32_t len, uint8_t *dst)
{
    const uint32_t r = len & 3u, sh = 2u * r;
    const int q = (int)(len >> 2);
    uint32_t prev = 0;
#pragma unroll
    for (int t = 0; t <= WALK_LS_WORDS; ++t) {
        const uint32_t cur = t < WALK_LS_WORDS ? st[t * 64] : 0u;
        const uint32_t S = __builtin_amdgcn_alignbit(cur, prev, sh);      // bases found as [16 (t - 1) + r, 16 t + r)
        prev = cur;
        const int w0 = q - 4 * t;                                         // S >> 24 -> word w0, ..., S & 0xff -> word w0 + 3
        if (t == 0) { if (r) *(uint32_t *)(dst + 4 * q) = walk_expand4(S >> 24) & ((1u << (8u * r)) - 1u); }
        else if (w0 >= 0) {
            WalkU4 v; v.x = walk_expand4(S >> 24); v.y = walk_expand4((S >> 16) & 0xffu); v.z = walk_expand4((S >> 8) & 0xffu); v.w = walk_expand4(S & 0xffu);
            *(WalkU4 *)(dst + 4 * w0) = v;
        } else if (w0 + 3 >= 0) {                                         // the sequence's first words: fewer than four
            if (w0 + 1 >= 0) *(uint32_t *)(dst + 4 * (w0 + 1)) = walk_expand4((S >> 16) & 0xffu);
            if (w0 + 2 >= 0) *(uint32_t *)(dst + 4 * (w0 + 2)) = walk_expand4((S >> 8) & 0xffu);
            *(uint32_t *)(dst + 4 * (w0 + 3)) = walk_expand4(S & 0xffu);
        }
    }
}

// MODE = WALK_HEAD: item t = admission record t (k_ovl_head_adm: the strand's row in ids[], park[] and rec[] and where its walk stands
// behind the tail table); the first 32 bases stay in registers and leave with the parked state in ONE 64-byte burst.
// MODE = WALK_TAIL: item = slot of the batch (rows of srev, listA), gidx[slot] = its row in park[], rec[] (and, for the kernels
// that follow, nei[] and seq[]).
// The fields of WalkArgs as parameters: members of a struct passed by value carry no __restrict__, and the compiler reads them again from the kernel-argument
// segment after every store and atomic (measured: + 4 VGPRs and 20 .. 36 bytes of scratch per lane in three of the four modes).
template <int MODE>
__device__ __forceinline__ void walk_run(const FmdIndexView &ix, size_t n, const uint64_t *__restrict__ ids, int min_match, int info_only,
                                         fmd_ovlp_rec_t *__restrict__ rec, uint8_t *__restrict__ srev, uint32_t stride_r,
                                         fmd_intv_t *__restrict__ listA, uint32_t cap, uint32_t *__restrict__ queue, uint32_t tickets,
                                         FmdWalkPark *__restrict__ park, const uint4 *__restrict__ adm, int pair_from,
                                         const uint32_t *__restrict__ gidx, uint8_t *__restrict__ seq_out, uint32_t seq_stride,
                                         uint32_t *__restrict__ redo, uint32_t *__restrict__ cls, int use_fast, int min_cls,
                                         const uint32_t *__restrict__ keys)
{
    FMD_DECLARE_COMPACT_LDS();
    __shared__ uint32_t walk_ls[MODE == WALK_TAIL2 ? 64 * WALK_LS_WORDS : 1];   // WALK_TAIL2: the lane's bases, word w of lane l at [w * 64 + l]
    constexpr bool TAILM = MODE == WALK_TAIL || MODE == WALK_TAIL2;
    constexpr int WAUX = MODE == WALK_HEAD ? FMD_HEAD_AUX : FMD_GLDS_AUX;   // pass 1 never asks for a line twice (strands in id order: every gather is a DRAM miss)
    size_t sid = 0;
    size_t gs = 0;                        // the strand's row in rec[] (WALK_TAIL: gidx[sid], otherwise sid)
    int st = WK_IDLE;
    uint32_t depth = 0, npush = 0, pack = 0, flags = 0;
    uint32_t pk0 = 0, pk1 = 0, pk2 = 0;   // the stash is written 16 bases at a time (one 16-byte store per lane instead of four words)
    uint64_t k = 0, x0 = 0, x1 = 0, sz = 0;
    bool exhausted = false;
    // The first ptab_d bases need no interval arithmetic when nothing can be pushed that early
    // (min_match >= ptab_d): LF steps only (one line each instead of three), the bi-interval then comes
    // from the prefix table -- forward string for x[0] and the size, reverse complement for x[1].
    const bool tab_ok = ix.ptab != nullptr && (info_only || min_match >= ix.ptab_d) && ix.ptab_d >= 2;
    bool tab = false;
    uint32_t tfw = 0, trv = 0;
    uint4 adm_a = make_uint4(0, 0, 0, 0), adm_b = make_uint4(0, 0, 0, 0);   // WALK_HEAD: the admission record of a strand on its way in (WK_ADM1)
    FmdTickets tk_;
    constexpr bool GUIDED = MODE != WALK_WHOLE;   // guided ticket chunks (fmd_wave.h) in the two passes of a sorted job, fixed ones in the one-pass walk
    // WALK_TAIL2 with the sorted keys at hand: the strands of one minimizer in phase on the genome (see WALK_TAIL2 above).  A generation is 64 consecutive
    // strands of the sorted order: fixed chunks of 64 tickets (fmd_launch_walk_tail2), since a guided chunk ends anywhere and the rest of the generation would
    // come from the chunk reserved ahead, somewhere else in the order
    const bool phase = MODE == WALK_TAIL2 && keys != nullptr;
    const size_t n_guided = GUIDED && !phase ? n : 0;
    fmd_tickets_init(tk_, queue, tickets, n_guided);
    for (;;) {
        int fin_cls = -1;                 // WALK_TAIL2 with the work lists of get_nei made here (cls != nullptr): the list of the strand this lane closes in this step
        if (MODE == WALK_TAIL2) {
            // The close of the strands that are through their right extension (WK_DONE): the record in one piece, the row in read order, the work list the
            // strand belongs on.  Free-running, a strand closes in the step after its last; in phase, the strands of a generation finish in up to 17
            // different steps, and walk_emit_row costs the wave its ~250 instructions whoever takes part: they close in company -- when half the wave
            // waits (the rule of k_ovl_nei_lane's full round) or nobody is walking any more.
            const uint64_t dn = __ballot(st == WK_DONE);
            if (dn && ((uint32_t)__popcll(dn) >= (phase ? 32u : 1u) || __ballot(st != WK_IDLE && st != WK_DONE) == 0)) {
                if (st == WK_DONE) {   // k = fm_retrieve's row, x0 = k[0], x1 and sz = the two '$' ranks of the right extension (k[1], k[2])
                    uint4 *o = (uint4 *)(rec + gs);
                    o[0] = make_uint4((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)x0, (uint32_t)(x0 >> 32));
                    o[1] = make_uint4((uint32_t)x1, (uint32_t)(x1 >> 32), (uint32_t)sz, (uint32_t)(sz >> 32));
                    o[2] = make_uint4(depth, (flags & WALK_F_CONTAINED) ? (uint32_t)-3 : 0u, npush, (uint32_t)-1);           // len, status, n_ovlp, rbeg
                    o[3] = make_uint4(0u, 0u, flags & ~WALK_F_INTERNAL, 2u);                               // ext_len, n_nei, flags, reserved = 2 | lfork = 0
                    // (the caller's copy in read order: from LDS a lane writes it without holding up the others; every sequence with a complete record
                    // gets its row -- k_ovl_seq_out's conditions)
                    if (flags & WALK_F_HASN) redo[1 + atomicAdd(redo, 1u)] = (uint32_t)sid;
                    else walk_emit_row(walk_ls + fmd_lane(), depth, seq_out + gs * (size_t)seq_stride);
                    if (cls != nullptr && !(flags & WALK_F_CONTAINED) && npush > 0 && !(flags & FMD_OVLP_F_OVERFLOW))   // (the strands k_ovl_classify takes from the records)
                        fin_cls = fmd_ovl_list_of(npush, depth, (flags & WALK_F_W63) != 0, (flags & WALK_F_WNARROW) != 0, (flags & WALK_F_W32) != 0, use_fast, min_cls);
                    st = WK_IDLE;
                }
            }
        }
        if (MODE == WALK_TAIL2 && cls != nullptr) {
            // k_ovl_classify's work, by the lanes that have just closed a strand: one returning atomic per
            // list that gets entries, all of them issued at once (lane j reserves for the j-th distinct list), then every lane writes its entry.  The lists
            // and counters are where ovl_phase_b expects them (`cls` = the area of the part: fmd_cls_list, fmd_cls_cnt_off); depth, npush and sid are still
            // the finished strand's.
            uint64_t rem = __ballot(fin_cls >= 0);
            if (rem) {
                const int lane = fmd_lane();
                int my_c = 0, nc = 0;
                uint32_t my_cnt = 0, my_slot = 0, my_rank = 0;
                while (rem) {
                    const int c = __builtin_amdgcn_readlane(fin_cls, __ffsll((unsigned long long)rem) - 1);
                    const uint64_t mk = __ballot(fin_cls == c);
                    if (lane == nc) { my_c = c; my_cnt = (uint32_t)__popcll(mk); }
                    if (fin_cls == c) { my_slot = (uint32_t)nc; my_rank = (uint32_t)fmd_below(mk); }
                    rem &= ~mk; ++nc;
                }
                uint32_t base = 0;
                if (lane < nc) base = atomicAdd(cls + fmd_cls_cnt_off(my_c) + FMD_CW_COUNT, my_cnt);
                base = (uint32_t)__shfl((int)base, (int)my_slot) + my_rank;
                if (fin_cls >= 0) {
                    uint32_t *lslow = fmd_cls_list(cls, FMD_CLS_SLOW, n);   // (n: the strands of this launch, i.e. of the part)
                    if (fin_cls == FMD_CLS_SLOW) lslow[base] = (uint32_t)sid;
                    else { uint32_t *lst = fmd_cls_list(cls, fin_cls, n); lst[2 * base] = (uint32_t)sid; lst[2 * base + 1] = npush | depth << 16; }
                    fin_cls = -1;
                }
            }
        }
        // in phase, a wave takes strands by generation: only when all its lanes are idle, one whole chunk of 64 tickets (lanes that find the queue drained stay idle)
        const bool gen_open = !phase || __ballot(st != WK_IDLE) == 0;
        const size_t my = fmd_tickets_take(tk_, queue, st == WK_IDLE && !exhausted && gen_open, n_guided);
        if (st == WK_IDLE && !exhausted && gen_open) {
            // The two passes of a sorted job take a strand in over one (WALK_HEAD) or two (WALK_TAIL) wave steps: the loads are issued
            // here and complete under the gather of the other lanes (WK_ADM1 / WK_ADM2 below).  A chain of dependent loads in front of
            // the gather -- id, tail-table entry, two prefix-table entries, as the one-pass walk does it -- stalls all 64 lanes of a wave
            // whose strands live 20 steps: k_ovl_head_adm resolves that chain for every strand beforehand, streaming.
            if (TAILM) {
                if (my < n) { sid = my; gs = gidx[my]; if (phase) pack = keys[my]; st = WK_ADM1; }   // (pack: nobody's until WK_ADM1 reads the parked line into it)
                else exhausted = true;
            } else if (MODE == WALK_HEAD) {
                if (my < n) { sid = my; adm_a = adm[2 * my]; adm_b = adm[2 * my + 1]; st = WK_ADM1; }
                else exhausted = true;
            } else
            if (my < n) {
                sid = my; gs = my; k = ids[gs]; depth = 0; npush = 0; pack = 0; pk0 = pk1 = pk2 = 0; flags = 0; st = WK_LF; tab = tab_ok;
                // the first ptab_d LF steps were taken when the index was loaded (FmdIndexView::tail): pick the walk up behind them
                const unsigned long long te = (tab_ok && ix.tail && k < ix.n_seq) ? ix.tail[k] : ~0ull;
                if (te != ~0ull) {
                    tfw = (uint32_t)(te >> (64 - 2 * ix.ptab_d)); k = te & ((1ull << (64 - 2 * ix.ptab_d)) - 1);
                    for (int jb = 0; jb < ix.ptab_d; ++jb) {   // the bases into the stash, as the steps would have put them
                        WALK_PUT_BASE(((tfw >> (2 * jb)) & 3u) + 1u);
                    }
                    // reverse complement of the ptab index: the 2-bit groups in reverse order, complemented
                    { uint32_t r = __brev(~tfw) >> (32 - 2 * ix.ptab_d); trv = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1); }
                    const uint4 ef = ix.ptab[tfw], er = ix.ptab[trv];
                    fmd_count_lane(ix, 2, 1);
                    x0 = (uint64_t)ef.y << 32 | ef.x;
                    sz = ((uint64_t)ef.w << 32 | ef.z) - x0 + 1;
                    x1 = (uint64_t)er.y << 32 | er.x;
                    tab = false;
                    st = walk_lf_shares(k, x0, sz) ? WK_BOTH : WK_LF;
                }
            }
            else exhausted = true;
        }
        if (__ballot(st != WK_IDLE) == 0) break;

        // ---- requests.  WK_LF: block of k only.  WK_EXT / WK_BOTH: the two ends of I's backward
        //      extension (k sits in one of them for WK_BOTH).  WK_RIGHT: forward '$' extension.
        uint64_t qk = NONE64, ql = NONE64;
        if (st == WK_LF) qk = k;
        else if (st == WK_EXT || st == WK_BOTH) { qk = x0 - 1; ql = x0 - 1 + sz; }
        else if (st == WK_RIGHT) { qk = x1 - 1; ql = x1 - 1 + sz; }
        FmdRank2c r = fmd_wave_rank2_fetch_compact<WAUX>(ix, fmd_lds, qk, ql);
        // two-phase step (more than 32 lanes straddle: wide intervals): the k-side ranks are taken now,
        // the l-side after fmd_wave_l_ready(); a narrow lane whose window straddles sits this step out
        uint64_t tk2[6] = {0, 0, 0, 0, 0, 0};
        const bool wide_ext = st == WK_EXT || (st == WK_BOTH && sz > 63);
        bool skip = false;
        if (r.two_phase) {
            if (wide_ext && r.hk) fmd_block_rank6<false>(r.bk, r.t, r.nk, tk2, r.blk_k);
            if (st == WK_RIGHT && r.hk) tk2[0] = fmd_block_rank1(r.bk, r.t, r.nk, 0, r.blk_k);
            { uint32_t ko_; skip = st == WK_BOTH && (sz <= 63 || !fmd_in_block(k, r.blk_k, ko_)) && r.l_sep; }
            if (st == WK_BOTH && sz > 63 && !skip) skip = true; // wide WK_BOTH never shares a gather in two-phase steps
            if (skip && st == WK_BOTH) st = WK_LF;   // take the LF step on its own next time, then the extension through the
                                                     // general path (a lane that merely waited could wait forever: the same
                                                     // lanes straddle again next step)
        }
        const bool was_two_phase = r.two_phase;
        fmd_wave_l_ready<WAUX>(ix, fmd_lds, r);
        if (st == WK_IDLE || skip || (MODE == WALK_TAIL2 && st == WK_DONE)) continue;
        if (MODE == WALK_TAIL2 && st == WK_WAIT) {   // a waiting lane posts no request and is not idle
            if (--npush == 0) st = walk_lf_shares(k, x0, sz) ? WK_BOTH : WK_LF;   // (npush: the countdown, 0 again when the walk starts)
            continue;
        }
        if (MODE == WALK_HEAD && st == WK_ADM1) {   // the admission record has arrived (FmdHeadAdm, k_ovl_head_adm)
            gs = adm_a.x;
            depth = 0; npush = 0; pack = 0; pk0 = pk1 = pk2 = 0; flags = 0;
            if (adm_b.w & 1u) {   // no tail-table entry: from the sentinel, on the ordinary path
                k = (uint64_t)(adm_b.y & 0xffu) << 32 | adm_a.y; st = WK_LF; tab = tab_ok;
            } else {
                const uint32_t hi = adm_b.y;
                k = (uint64_t)(hi & 0xffu) << 32 | adm_a.y; x0 = (uint64_t)((hi >> 8) & 0xffu) << 32 | adm_a.z;
                x1 = (uint64_t)((hi >> 16) & 0xffu) << 32 | adm_a.w; sz = (uint64_t)(hi >> 24) << 32 | adm_b.x;
                // the ptab_d bases of the tail as nibbles (2-bit code + 1): 8 per word
                const uint32_t tf = adm_b.z;
                uint32_t lo = tf & 0xffffu, up = tf >> 16;
                lo = (lo | lo << 8) & 0x00ff00ffu; lo = (lo | lo << 4) & 0x0f0f0f0fu; lo = (lo | lo << 2) & 0x33333333u;
                up = (up | up << 8) & 0x00ff00ffu; up = (up | up << 4) & 0x0f0f0f0fu; up = (up | up << 2) & 0x33333333u;
                const int d = ix.ptab_d;
                pk0 = (lo + 0x11111111u) & (d >= 8 ? ~0u : (1u << (4 * d)) - 1u);
                pk1 = d > 8 ? (up + 0x11111111u) & (d >= 16 ? ~0u : (1u << (4 * (d - 8))) - 1u) : 0u;
                depth = (uint32_t)d; tab = false;
                st = walk_lf_shares(k, x0, sz) ? WK_BOTH : WK_LF;
            }
            continue;
        }
        if (TAILM && st == WK_ADM1) {   // the strand's row is known: fetch what WALK_HEAD parked there, straight into the
            const uint4 *pp = (const uint4 *)(park + gs);   // registers the state will live in (the loads land under the next gather)
            const uint4 a = pp[0], b = pp[1], cb = pp[2];
            k = (uint64_t)a.y << 32 | a.x; x0 = (uint64_t)a.w << 32 | a.z; x1 = (uint64_t)b.y << 32 | b.x; sz = (uint64_t)b.w << 32 | b.z;
            // (WALK_TAIL2 has no stash registers of its own: the parked bases wait one step in npush, depth and flags, which belong to nobody until WK_ADM2 sets
            // all three.  NOTHING may read depth, npush or flags of a lane in WK_ADM2.  It buys three VGPRs: 125 with it, 128 -- the limit, nothing spilled --
            // with pk0..2 carried instead (tools/kernel_resources.py), so it can be undone as long as nothing else wants those three.)
            // In phase, pack holds the strand's sort key since the ticket: what WK_ADM2 needs of it moves into the spare bits of st before the line takes pack.
            st = WK_ADM2;
            if (MODE == WALK_TAIL2 && phase) st |= (int)((pack & 31u) | (pack < 0xfffffffeu ? 32u : 0u)) << WK_KEY_SHIFT;
            if (MODE == WALK_TAIL2) { npush = cb.x; depth = cb.y; flags = cb.z; pack = cb.w; }
            else { pk0 = cb.x; pk1 = cb.y; pk2 = cb.z; pack = cb.w; }
            continue;
        }
        if (MODE == WALK_TAIL2 && (st & WK_STATE_MASK) == WK_ADM2) {
            // The lanes of a generation arrive here together.  A strand whose minimizer lies o bases from its end waits omax - o steps, omax the largest
            // offset of the generation: from then on every strand of a key stands at the same genome position in every step.  A key without a
            // minimizer (k_ovl_park_keys) waits for nobody.
            uint32_t wait = 0;
            if (phase) {
                const uint32_t kb = (uint32_t)st >> WK_KEY_SHIFT, o = kb & 31u;
                const bool has = (kb & 32u) != 0;
                uint64_t top = __ballot(has);
                uint32_t omax = 0;
#pragma unroll
                for (int b = 4; b >= 0; --b) {
                    const uint64_t m = __ballot(has && ((o >> b) & 1u)) & top;
                    if (m) { top = m; omax |= 1u << b; }
                }
                wait = has ? omax - o : 0u;
            }
            st = WK_IDLE;
            if (k != ~0ull) {   // (~0: the sequence ended inside the head)
                const uint32_t c0 = walk_nib_to_2bit(npush), c1 = walk_nib_to_2bit(depth), c2 = walk_nib_to_2bit(flags), c3 = walk_nib_to_2bit(pack);
                walk_ls[fmd_lane()] = (c0 & 0xffffu) | c1 << 16; walk_ls[64 + fmd_lane()] = (c2 & 0xffffu) | c3 << 16;
                depth = FMD_WALK_SPLIT; npush = wait; pack = 0; tab = false;
                flags = ((c0 | c1 | c2 | c3) & 0x10000u) ? WALK_F_HASN : 0u;
                st = wait ? WK_WAIT : walk_lf_shares(k, x0, sz) ? WK_BOTH : WK_LF;
            }
            continue;
        }
        if (MODE == WALK_TAIL && st == WK_ADM2) {
            st = WK_IDLE;
            if (k != ~0ull) {   // (~0: the sequence ended inside the head)
                uint4 *sr = (uint4 *)(srev + sid * (size_t)stride_r);   // the 32 bases into the stash, one per byte
#define WALK_NIB4(v_) (((v_) & 0xfu) | ((v_) & 0xf0u) << 4 | ((v_) & 0xf00u) << 8 | ((v_) & 0xf000u) << 12)
                sr[0] = make_uint4(WALK_NIB4(pk0), WALK_NIB4(pk0 >> 16), WALK_NIB4(pk1), WALK_NIB4(pk1 >> 16));
                sr[1] = make_uint4(WALK_NIB4(pk2), WALK_NIB4(pk2 >> 16), WALK_NIB4(pack), WALK_NIB4(pack >> 16));
#undef WALK_NIB4
                depth = FMD_WALK_SPLIT; npush = 0; pack = 0; pk0 = pk1 = pk2 = 0; flags = 0; tab = false;
                st = walk_lf_shares(k, x0, sz) ? WK_BOTH : WK_LF;
            }
            continue;
        }

        int c = (int)((flags & WALK_F_CPEND) >> WALK_F_CPEND_SHIFT);
        // Narrow interval (size <= 63, i.e. all but the first ~log4(n) bases): everything comes from ONE
        // 64-position window of BWT[x0, x0+size) read out of the lane's block image -- the six child
        // sizes, the base at row k (k lies inside the window) and rank_c(k) -- plus ONE absolute rank
        // of ONE symbol, rank_c(x0-1).  ~150 VALU instead of two full six-symbol block ranks (~600).
        const bool narrow = st == WK_BOTH && sz <= 63;
        // What the rest of the turn needs of it: the sizes of child 0 and of child c = BWT[k], the sizes ordered before c (0 < 4 < 3 < 2 < 1 < 5) and where
        // child c starts (cnt[c] + rank_c(x0 - 1); cnt[0] = 0) -- all of them popcounts of masks over the window.
        // Two widths, ONE of them per wave step: while no narrow lane of the wave is wider than 31 (pass 2 of 30-fold reads: nearly every step) the window
        // BWT[x0, x0 + size) starts at offset 1 .. 64 of the block of x0 - 1 and ends inside its 96 positions: two chunks of that one image, 32-bit masks, and
        // the rank from the chunks already in registers.  Otherwise the 64-position window over both images.
        uint32_t ns0 = 0, nsc = 0, nbef = 0;
        uint64_t nx0 = 0, wD = 0, wr0 = 0;  // wD, wr0: the narrow form of cand_store (fmd_kernel_common.h)
        if (narrow) {
            if (__ballot(sz > 31) == 0) {
                const uint32_t ch = r.nk >> 5, sh = r.nk & 31;               // r.nk = offset of x0 in the block of x0 - 1: 1 .. 64
                const uint4 v0 = r.bk[0 ^ r.t], v1 = r.bk[1 ^ r.t], v2 = r.bk[2 ^ r.t], mv = r.bk[3 ^ r.t];   // the image, once
                // the window's chunks ch and min(ch + 1, 2) out of the registers (ch = 2: offset 64, shift 0 -- the second word is not looked at)
                uint4 a = v0, b = v1;
                a.x = ch == 1 ? v1.x : a.x; a.y = ch == 1 ? v1.y : a.y; a.z = ch == 1 ? v1.z : a.z;
                a.x = ch == 2 ? v2.x : a.x; a.y = ch == 2 ? v2.y : a.y; a.z = ch == 2 ? v2.z : a.z;
                b.x = ch != 0 ? v2.x : b.x; b.y = ch != 0 ? v2.y : b.y; b.z = ch != 0 ? v2.z : b.z;
                const uint32_t m2 = v2.w;
                const uint32_t X = __builtin_amdgcn_alignbit(b.x, a.x, sh), Y = __builtin_amdgcn_alignbit(b.y, a.y, sh), Z = __builtin_amdgcn_alignbit(b.z, a.z, sh);
                const uint32_t m = (1u << (uint32_t)sz) - 1u;
                const uint32_t o = (uint32_t)k - (uint32_t)x0;               // row k inside the window
                const uint32_t ex = ((X >> o) & 1u) - 1u, ey = ((Y >> o) & 1u) - 1u, ez = ((Z >> o) & 1u) - 1u;   // all ones where the bit of c is clear
                c = (int)((~ex & 1u) | (~ey & 2u) | (~ez & 4u));
                const uint32_t M0 = ~(X | Y | Z) & m, Mc = (X ^ ex) & (Y ^ ey) & (Z ^ ez) & m;
                const uint32_t Mb = win_before(X, Y, Z, ~ex, ~ey, ~ez) & m;
                ns0 = (uint32_t)__builtin_popcount(M0); nsc = (uint32_t)__builtin_popcount(Mc); nbef = (uint32_t)__builtin_popcount(Mb);
                nx0 = walk_cnt(ix, c) + fmd_block_rank1z_regs(v0, v1, m2, mv, r.nk, c, ex, ey, ez, r.blk_k, wr0);   // rank_c(x0 - 1), rank_$(x0 - 1)
                wD = M0;
                k = nx0 + (uint32_t)__builtin_popcount(Mc & ((2u << o) - 1u)) - 1;
            } else {
                const uint32_t sh = (uint32_t)x0 & 31;
                uint4 a, b, cc;
                grp_window(r.bk, r.t, r.bl, r.tl, r.blk_k, r.blk_l, r.hk, r.l_sep, r.blk_k, r.nk - 1, a, b, cc); // window at x0 = (x0 - 1) + 1
                const uint64_t m = bits_below((int)sz);
                const uint64_t X = win64(a.x, b.x, cc.x, sh), Y = win64(a.y, b.y, cc.y, sh), Z = win64(a.z, b.z, cc.z, sh);
                const uint32_t o = (uint32_t)(k - x0);                       // row k inside the window
                const uint64_t ex = ((X >> o) & 1) - 1, ey = ((Y >> o) & 1) - 1, ez = ((Z >> o) & 1) - 1;   // all ones where the bit of c is clear
                c = (int)(((uint32_t)~ex & 1u) | ((uint32_t)~ey & 2u) | ((uint32_t)~ez & 4u));
                const uint64_t M0 = ~(X | Y | Z) & m, Mc = (X ^ ex) & (Y ^ ey) & (Z ^ ez) & m;
                const uint64_t Mb = win_before(X, Y, Z, ~ex, ~ey, ~ez) & m;
                ns0 = (uint32_t)__popcll(M0); nsc = (uint32_t)__popcll(Mc); nbef = (uint32_t)__popcll(Mb);
                nx0 = walk_cnt(ix, c) + fmd_block_rank1z(r.bk, r.t, r.nk, c, r.blk_k, wr0);          // rank_c(x0 - 1), rank_$(x0 - 1)
                wD = M0;
                k = nx0 + __popcll(Mc & bits_below((int)o + 1)) - 1;
            }
        } else if (st == WK_LF || st == WK_BOTH) { // LF step at row k: base = BWT[k], k' = cnt[c] + rank_c(k) - 1
            uint32_t kb_ = r.blk_k, off;
            const bool in_k = fmd_in_block(k, r.blk_k, off);     // (WK_LF: the block asked for; WK_BOTH: one of the extension's two)
            if (!in_k) { kb_ = r.blk_l; fmd_in_block(k, r.blk_l, off); }
            const uint4 *img = in_k ? r.bk : r.bl;
            const int tt = in_k ? r.t : r.tl;
            const uint4 v = img[(int)(off >> 5) ^ tt];
            const uint32_t bit = off & 31;
            c = (int)(((v.x >> bit) & 1) | ((v.y >> bit) & 1) << 1 | ((v.z >> bit) & 1) << 2);
            k = walk_cnt(ix, c) + fmd_block_rank1(img, tt, off + 1, c, kb_) - 1;
            if (st == WK_LF && depth > 0 && tab) { // still inside the prefix table: no extension, just collect the base
                if (c < 1 || c > 4) { // the sequence ends, or an ambiguous base: start over on the ordinary path
                    k = ids[gs]; depth = 0; pack = 0; pk0 = pk1 = pk2 = 0; tab = false;
                    continue;
                }
                tfw |= (uint32_t)(c - 1) << (2 * depth); trv = trv << 2 | (uint32_t)(4 - c);
                WALK_PUT_BASE(c);
                if ((int)depth == ix.ptab_d) {
                    const uint4 ef = ix.ptab[tfw], er = ix.ptab[trv];
                    fmd_count_lane(ix, 2, 1);
                    x0 = (uint64_t)ef.y << 32 | ef.x;
                    sz = ((uint64_t)ef.w << 32 | ef.z) - x0 + 1;   // never empty: the sequence is in the index
                    x1 = (uint64_t)er.y << 32 | er.x;
                    tab = false;
                    st = walk_lf_shares(k, x0, sz) ? WK_BOTH : WK_LF;
                }
                continue;
            }
            if (st == WK_LF && depth > 0) { flags = (flags & ~WALK_F_CPEND) | (uint32_t)c << WALK_F_CPEND_SHIFT; st = WK_EXT; continue; } // the extension needs its own gather
        }
        if (depth == 0) { // first LF step: the last base of the sequence, or an empty sequence
            if (c == 0) {
                fmd_ovlp_rec_t *o = rec + gs;
                o->rank = k; o->k[0] = o->k[1] = o->k[2] = 0; o->len = 0; o->status = -1; o->n_ovlp = 0; o->rbeg = -1;
                o->ext_len = 0; o->n_nei = 0; o->flags = 0; o->reserved = 2; o->lfork = 0;
                if (MODE == WALK_HEAD) park[gs].k = ~0ull;
                st = WK_IDLE;
                continue;
            }
            x0 = ix.cnt[c]; x1 = ix.cnt[comp6(c)]; sz = ix.cnt[c + 1] - ix.cnt[c];
            WALK_PUT_BASE(c);   // (depth 0 -> 1)
            if (c > 4) tab = false;
            tfw = (uint32_t)(c - 1) & 3; trv = (uint32_t)(4 - c) & 3;
        } else if (st == WK_EXT || st == WK_BOTH) {
            // s0, sc: the sizes of child 0 and child c; before: the sizes ordered before c (0 < 4 < 3 < 2 < 1 < 5); nx: where child c starts
            uint64_t s0 = ns0, sc = nsc, before = nbef, nx = nx0;
            if (!narrow) {
                uint64_t tk[6] = {0, 0, 0, 0, 0, 0}, s[6];
                uint64_t tl[6] = {0, 0, 0, 0, 0, 0};
                if (was_two_phase) {
#pragma unroll
                    for (int a = 0; a < 6; ++a) tk[a] = tk2[a];
                } else if (r.hk) fmd_block_rank6<false>(r.bk, r.t, r.nk, tk, r.blk_k);
                if (r.hl) fmd_block_rank6<false>(r.bl, r.tl, r.nl, tl, r.blk_l);
#pragma unroll
                for (int a = 0; a < 6; ++a) s[a] = tl[a] - tk[a];
                s0 = s[0]; sc = sel6(c, s[0], s[1], s[2], s[3], s[4], s[5]);
                nx = walk_cnt(ix, c) + sel6(c, tk[0], tk[1], tk[2], tk[3], tk[4], tk[5]);
                before = s[0];
                if (c == 3 || c == 2 || c == 1 || c == 5) before += s[4];
                if (c == 2 || c == 1 || c == 5) before += s[3];
                if (c == 1 || c == 5) before += s[2];
                if (c == 5) before += s[1];
            }
            if (c != 0) { // one more base: overlap_intv's loop body (unitig.c:47-59)
                // (sc == 0 cannot happen: the sequence itself is in the index)
                if (MODE != WALK_HEAD && !info_only && (int)depth >= min_match && s0) {
                    if (npush < cap) {
                        fmd_intv_t *e = listA + sid * (size_t)cap + (cap - 1 - npush);
                        const bool nf = narrow && depth < 65536u;
                        cand_store(e, nf, x0, x1, sz, depth, wD, wr0);
                        if (MODE == WALK_TAIL2 && npush == 0)
                            flags |= (sz <= 63 ? WALK_F_W63 : 0u) | (nf ? WALK_F_WNARROW : 0u) | (sz > 31 ? WALK_F_W32 : 0u);
                    } else flags |= FMD_OVLP_F_OVERFLOW;
                    ++npush;
                }
                x0 = nx; x1 += before; sz = sc;
                WALK_PUT_BASE(c);
            } else { // '$': the sequence is complete (len = depth); these ranks are the left test of fm6_is_contained
                if (MODE == WALK_TAIL2) {
                    if ((depth & 15) && depth <= WALK_LS_BASES) walk_ls[(depth >> 4) * 64 + fmd_lane()] = pack;   // the last, partial word
                } else
                if (MODE != WALK_HEAD && (depth & 15) && depth <= stride_r) // the last, partial group of 16 (stride_r is a multiple of 16)
                {   // completed words of the group sit in pk0..2, a partial word in pack; everything past it is zero
                    const uint32_t wq = (depth >> 2) & 3;
                    *(uint4 *)(srev + sid * (size_t)stride_r + (depth & ~15u)) = make_uint4(wq == 0 ? pack : pk0, wq == 1 ? pack : pk1, wq == 2 ? pack : pk2, wq == 3 ? pack : 0u);
                }
                fmd_ovlp_rec_t *o = rec + gs;
                // (WALK_TAIL2 writes the record once, at the strand's close; here only the record of a strand that ends now)
                if (MODE != WALK_TAIL2 || depth > stride_r || (!info_only && (int)depth <= min_match)) {
                    o->rank = k; o->len = (int32_t)depth; o->rbeg = -1; o->ext_len = 0; o->n_nei = 0; o->reserved = 2; o->lfork = 0;
                    o->k[0] = o->k[1] = o->k[2] = 0; o->n_ovlp = 0;
                }
                if (MODE == WALK_HEAD) park[gs].k = ~0ull;   // ended inside the head: shorter than min_match, the record below is final
                if (depth > stride_r) { o->status = 0; o->flags = FMD_OVLP_F_OVERFLOW; st = WK_IDLE; continue; } // longer than max_len
                if (!info_only && (int)depth <= min_match) { o->status = -1; o->flags = 0; st = WK_IDLE; continue; } // too short (unitig.c:288)
                // (the caller's copy in read order is made by k_ovl_seq_out: a lane doing it here, from a stash in HBM, holds up the other 63;
                // WALK_TAIL2 writes it from LDS at the strand's close)
                if (sz != s0) flags |= WALK_F_CONTAINED;           // left-contained
                x0 = nx; sz = s0;                  // ok[0]: x[0] = cnt[0] + tk[0] (cnt[0] = 0), x[1] unchanged
                st = WK_RIGHT;
                continue;
            }
        } else if (st == WK_RIGHT) { // extend by '$' on the right (unitig.c:86-89)
            const uint64_t t0k = was_two_phase ? tk2[0] : (r.hk ? fmd_block_rank1(r.bk, r.t, r.nk, 0, r.blk_k) : 0);
            const uint64_t t0l = r.hl ? fmd_block_rank1(r.bl, r.tl, r.nl, 0, r.blk_l) : 0;
            if (sz != t0l - t0k) flags |= WALK_F_CONTAINED;
            if (MODE == WALK_TAIL2) { x1 = t0k; sz = t0l - t0k; st = WK_DONE; continue; }   // everything else at the close (top of the loop)
            fmd_ovlp_rec_t *o = rec + gs;
            o->k[0] = x0; o->k[1] = t0k; o->k[2] = t0l - t0k;
            o->status = (flags & WALK_F_CONTAINED) ? -3 : 0;
            o->n_ovlp = (int32_t)npush;
            o->flags = flags & ~WALK_F_INTERNAL;
            st = WK_IDLE;
            continue;
        }
        // next base: can the LF step share the extension's gather?
        {
            st = walk_lf_shares(k, x0, sz) ? WK_BOTH : WK_LF;
            if (tab) st = WK_LF;   // inside the prefix table there is no extension to share a gather with
        }
        // park the strand: one 64-byte line, written whole.  pair_from: a depth below FMD_WALK_SPLIT at which the head hands the strand to
        // k_ovl_pair (two bases per request from there on; pad.w >> 24 = that depth), 0 = FMD_WALK_SPLIT, the strand parked for good
        // (Handing a strand over at the first even depth at which its interval is narrow -- 63 % of the strands of 30-fold reads at 14, nearly all at 16 -- was
        // measured and not kept: the head's time is its first two, wide, bases, and k_ovl_pair lost more than the head gained: 36.3 -> 39.3 ms, profiles/r6_pair.)
        // A strand whose interval is still wider than 63 at the hand-over is not handed over: it goes on here, one base at a time, and is parked for good.
        if (MODE == WALK_HEAD && !tab && (depth == FMD_WALK_SPLIT || (pair_from > 0 && depth == (uint32_t)pair_from && sz <= 63))) {
            uint4 *pp = (uint4 *)(park + gs);
            pp[0] = make_uint4((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)x0, (uint32_t)(x0 >> 32));
            pp[1] = make_uint4((uint32_t)x1, (uint32_t)(x1 >> 32), (uint32_t)sz, (uint32_t)(sz >> 32));
            pp[2] = make_uint4(pk0, pk1, pk2, pack); pp[3] = make_uint4(0, 0, 0, depth < FMD_WALK_SPLIT ? depth << 24 : 0u);
            st = WK_IDLE;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(64, 4) void k_ovl_walk(const WalkArgs a)
{
    walk_run<MODE>(a.ix, a.n, a.ids, a.min_match, a.info_only, a.rec, a.srev, a.stride_r, a.listA, a.cap, a.queue, a.tickets, a.park, a.adm, a.pair_from,
                   a.gidx, a.seq_out, a.seq_stride, a.redo, a.cls, a.use_fast, a.min_cls, a.keys);
}

#undef WALK_STASH_WORD
#undef WALK_PUT_BASE

// ---- two bases per request (round 6; fmd_pair.hip, fmd_wave.h) -----------------------------------------------------------------------
// Pass 1 of a sorted job below FMD_WALK_SPLIT, for an index that has two-base blocks: WALK_HEAD takes every strand to depth `from` (16: by then the
// interval of a strand of 30-fold reads is narrower than 64) and parks it; this kernel takes it on to FMD_WALK_SPLIT two bases per gather and parks it
// for good.  It does NOTHING else -- no single steps, no wide intervals, no sequence ends: a strand it cannot take all the way (an interval still wider than
// 63, an N or the sequence's end within the next two bases) goes on a list, and WALK_HEAD walks those again from their admission records.  That is
// what keeps it lean: one 8 KiB landing slot and ~70 registers per wave, so that a CU holds as many waves as the single-step head -- the first form of
// this (k_ovl_walk<WALK_HEADP>, profiles/r6_pair) carried the whole single-step engine beside the pair step, held 8 waves per CU and lost.
// A pair block starts every 32 positions and describes 96: an interval of up to 64 positions lies inside the block of its first position.
// The step: the positions of the window with first symbol c1 are the interval one base on, in order; those among them with second symbol c2 the interval
// two bases on: sizes, the x[1] sums of both extensions (fm6_extend's order 0 < 4 < 3 < 2 < 1 < 5, exact.c:81-86) and the rank of row k are popcounts,
// the start is one pair count (block + superblock: ix.pair_tab, which also holds K2[c1][c2] = cnt[c2] + #{c2 in BWT[0, cnt[c1])}).
enum { PK_IDLE = 0, PK_LOAD, PK_RUN };
#ifndef FMD_PAIR_AUX
#define FMD_PAIR_AUX FMD_HEAD_AUX      // cache-policy bits of the two-base gather (2 = nt: every line is asked for once)
#endif
#ifndef FMD_PAIR_LB
#define FMD_PAIR_LB 4                  // waves per SIMD the kernel is compiled for
#endif
__global__ __launch_bounds__(64, FMD_PAIR_LB) void k_ovl_pair(FmdIndexView ix, size_t n, FmdWalkPark *__restrict__ park, uint32_t *__restrict__ queue, uint32_t tchunk,
                                                  uint32_t *__restrict__ strag)
{
    __shared__ uint4 pair_lds[FMD_PAIR_SLOT_U4];
    const int q_ = fmd_lane(), px = fmd_pair_xor(q_);
    const uint4 *img = pair_lds + fmd_pair_base(q_);
    const uint32_t *iw = (const uint32_t *)img;
    size_t row = 0;
    int st = PK_IDLE;
    bool exhausted = false;
    uint32_t depth = 0, pk0 = 0, pk1 = 0, pk2 = 0, pk3 = 0;
    uint64_t k = 0, x0 = 0, x1 = 0, sz = 0;
    uint4 la = make_uint4(0, 0, 0, 0), lb = la, lc = la, ld = la;
    FmdTickets tk_;
    fmd_tickets_init(tk_, queue, tchunk, n);   // (guided chunks)
    for (;;) {
        const size_t my = fmd_tickets_take(tk_, queue, st == PK_IDLE && !exhausted, n);
        if (st == PK_IDLE && !exhausted) {
            if (my < n) {   // the parked line: its loads land under the gather of the other lanes
                row = my;
                const uint4 *pp = (const uint4 *)(park + row);
                la = pp[0]; lb = pp[1]; lc = pp[2]; ld = pp[3];
                st = PK_LOAD;
            } else exhausted = true;
        }
        if (__ballot(st != PK_IDLE) == 0) break;
        fmd_pair_fetch<FMD_PAIR_AUX>(ix, pair_lds, (uint32_t)(x0 >> 5), st == PK_RUN);
        fmd_fetch_wait();
        if (st == PK_LOAD) {
            k = (uint64_t)la.y << 32 | la.x; x0 = (uint64_t)la.w << 32 | la.z; x1 = (uint64_t)lb.y << 32 | lb.x; sz = (uint64_t)lb.w << 32 | lb.z;
            pk0 = lc.x; pk1 = lc.y; pk2 = lc.z; pk3 = lc.w;
            depth = ld.w >> 24;
            st = PK_RUN;
            if (k == ~0ull || depth == 0) st = PK_IDLE;                        // the sequence ended inside the head / the strand is parked for good already
            else if (sz > 63 || depth + 2 > FMD_WALK_SPLIT) { strag[1 + atomicAdd(strag, 1u)] = (uint32_t)row; st = PK_IDLE; }
            continue;
        }
        if (st != PK_RUN) continue;
        const uint32_t off = (uint32_t)x0 & 31u;
        const uint4 A0 = img[0 ^ px], A1 = img[1 ^ px], A2 = img[2 ^ px], B0 = img[3 ^ px], B1 = img[4 ^ px], B2 = img[5 ^ px];
        const uint64_t X = win64(A0.x, A1.x, A2.x, off), Y = win64(A0.y, A1.y, A2.y, off), Z = win64(A0.z, A1.z, A2.z, off);
        const uint64_t S0 = win64(A0.w, A1.w, A2.w, off), S1 = win64(B0.x, B1.x, B2.x, off), S2 = win64(B0.y, B1.y, B2.y, off);
        const uint64_t m = bits_below((int)sz);
        const uint32_t o = (uint32_t)(k - x0);
        const int c1 = (int)(((X >> o) & 1) | ((Y >> o) & 1) << 1 | ((Z >> o) & 1) << 2);
        const int c2 = (int)(((S0 >> o) & 1) | ((S1 >> o) & 1) << 1 | ((S2 >> o) & 1) << 2);
        if (c1 < 1 || c1 > 4 || c2 < 1 || c2 > 4) { strag[1 + atomicAdd(strag, 1u)] = (uint32_t)row; st = PK_IDLE; continue; }   // the sequence ends within two bases, or an N
        const uint64_t lo = ~Z & m, hi = Z & ~Y & m;
        const uint64_t M0 = lo & ~Y & ~X, M1 = lo & ~Y & X, M2 = lo & Y & ~X, M3 = lo & Y & X, M4 = hi & ~X;
        const uint64_t Mc = c1 == 1 ? M1 : c1 == 2 ? M2 : c1 == 3 ? M3 : M4;
        const uint64_t lo2 = ~S2 & Mc, hi2 = S2 & ~S1 & Mc;
        const uint64_t N0 = lo2 & ~S1 & ~S0, N1 = lo2 & ~S1 & S0, N2 = lo2 & S1 & ~S0, N3 = lo2 & S1 & S0, N4 = hi2 & ~S0;
        const uint64_t Mp = c2 == 1 ? N1 : c2 == 2 ? N2 : c2 == 3 ? N3 : N4;
        uint32_t before = (uint32_t)__popcll(M0) + (uint32_t)__popcll(N0);          // '$' sorts before every base
        if (c1 != 4) before += (uint32_t)__popcll(M4);
        if (c1 == 2 || c1 == 1) before += (uint32_t)__popcll(M3);
        if (c1 == 1) before += (uint32_t)__popcll(M2);
        if (c2 != 4) before += (uint32_t)__popcll(N4);
        if (c2 == 2 || c2 == 1) before += (uint32_t)__popcll(N3);
        if (c2 == 1) before += (uint32_t)__popcll(N2);
        // pairs (c1, c2) before x0: the superblock's (+ K2), the block's 28-bit count, positions [0, off) of the block's own chunk
        const uint32_t e0x = (c1 & 1) ? 0u : ~0u, e0y = (c1 & 2) ? 0u : ~0u, e0z = (c1 & 4) ? 0u : ~0u;
        const uint32_t e1x = (c2 & 1) ? 0u : ~0u, e1y = (c2 & 2) ? 0u : ~0u, e1z = (c2 & 4) ? 0u : ~0u;
        const uint32_t pm0 = (A0.x ^ e0x) & (A0.y ^ e0y) & (A0.z ^ e0z) & (A0.w ^ e1x) & (B0.x ^ e1y) & (B0.y ^ e1z);
        const uint32_t nb_ = (uint32_t)__builtin_popcount(pm0 & fmd_mask32((int)off));
        const int pr = 4 * (c1 - 1) + (c2 - 1), bp = 28 * pr, tw = bp >> 5, tw1 = tw < 13 ? tw + 1 : 13;
#define WP_CW(t) iw[(((t) < 6 ? 3 + ((t) >> 1) : 6 + (((t) - 6) >> 2)) ^ px) * 4 + ((t) < 6 ? 2 + ((t) & 1) : (((t) - 6) & 3))]
        const uint32_t cwl = WP_CW(tw), cwh = WP_CW(tw1);
#undef WP_CW
        const uint32_t rel = __builtin_amdgcn_alignbit(cwh, cwl, (uint32_t)bp & 31u) & 0x0fffffffu;
        const uint64_t base = ix.pair_tab[(x0 >> (5 + FMD_PAIR_SB_SHIFT)) * 16 + (uint64_t)pr];
        const uint64_t nx0 = base + rel + nb_;
        k = nx0 + (uint64_t)__popcll(Mp & bits_below((int)o + 1)) - 1;
        x0 = nx0; sz = (uint64_t)__popcll(Mp); x1 += before;
        {   // the two bases into the parked nibbles (FmdWalkPark::bases: 4 bits each, the sequence's last base first)
            const uint32_t v1 = (uint32_t)c1 << (4 * (depth & 7)), w1 = depth >> 3;
            pk0 |= w1 == 0 ? v1 : 0u; pk1 |= w1 == 1 ? v1 : 0u; pk2 |= w1 == 2 ? v1 : 0u; pk3 |= w1 == 3 ? v1 : 0u;
            const uint32_t d2 = depth + 1, v2 = (uint32_t)c2 << (4 * (d2 & 7)), w2 = d2 >> 3;
            pk0 |= w2 == 0 ? v2 : 0u; pk1 |= w2 == 1 ? v2 : 0u; pk2 |= w2 == 2 ? v2 : 0u; pk3 |= w2 == 3 ? v2 : 0u;
            depth += 2;
        }
        if (depth >= FMD_WALK_SPLIT) {   // parked for good: the line WALK_HEAD would have written
            uint4 *pp = (uint4 *)(park + row);
            pp[0] = make_uint4((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)x0, (uint32_t)(x0 >> 32));
            pp[1] = make_uint4((uint32_t)x1, (uint32_t)(x1 >> 32), (uint32_t)sz, (uint32_t)(sz >> 32));
            pp[2] = make_uint4(pk0, pk1, pk2, pk3); pp[3] = make_uint4(0, 0, 0, 0);
            st = PK_IDLE;
        } else if (sz > 63 || depth + 2 > FMD_WALK_SPLIT) { strag[1 + atomicAdd(strag, 1u)] = (uint32_t)row; st = PK_IDLE; }   // (cannot happen from an even depth with a narrow interval: sizes only shrink)
    }
}
// the admission records of the strands k_ovl_pair could not take all the way, for a second launch of WALK_HEAD
__global__ void k_ovl_strag_adm(const uint32_t *__restrict__ strag, const uint4 *__restrict__ adm, uint4 *__restrict__ adm2)
{
    const uint32_t n = strag[0];
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const size_t r = strag[1 + j];
        adm2[2 * (size_t)j] = adm[2 * r]; adm2[2 * (size_t)j + 1] = adm[2 * r + 1];
    }
}

// WALK_TAIL2's strands with an N (redo[0] of them, slots redo[1 ..]): one lane per strand, the row byte by byte -- the 32 bases WALK_HEAD parked, then LF steps from
// the parked row on, read straight from the index (no wave gather: a handful of strands per batch of real reads, none of synthetic ones).
__global__ void k_ovl_seq_redo(FmdIndexView ix, const uint32_t *__restrict__ redo, const uint32_t *__restrict__ gidx, const FmdWalkPark *__restrict__ park,
                               const fmd_ovlp_rec_t *__restrict__ rec, uint8_t *__restrict__ seq_out, uint32_t seq_stride)
{
    const uint32_t n = redo[0];
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const size_t g = gidx[redo[1 + j]];
        const int len = rec[g].len;
        uint8_t *dst = seq_out + g * (size_t)seq_stride;
        const uint4 *pp = (const uint4 *)(park + g);
        const uint4 a = pp[0], cb = pp[2];
        const uint32_t nib[4] = {cb.x, cb.y, cb.z, cb.w};
        uint64_t k = (uint64_t)a.y << 32 | a.x;
        for (int f = 0; f < (int)FMD_WALK_SPLIT && f < len; ++f) dst[len - 1 - f] = (uint8_t)((nib[f >> 3] >> (4 * (f & 7))) & 0xfu);
        for (int f = (int)FMD_WALK_SPLIT; f < len; ++f) {
            uint32_t b, o;
            fmd_split(k, b, o);
            const uint4 *img = ix.blocks + (size_t)b * FMD_BLK_U4;
            const uint4 v = img[o >> 5];
            const uint32_t bit = o & 31;
            const int c = (int)(((v.x >> bit) & 1) | ((v.y >> bit) & 1) << 1 | ((v.z >> bit) & 1) << 2);
            dst[len - 1 - f] = (uint8_t)c;
            k = ix.cnt[c] + fmd_block_rank1(img, 0, o + 1, c, b) - 1;
        }
    }
}

// The caller's copy of every sequence in read order: the stash holds it last base first.  One thread per 16 output bytes (four aligned
// dwords of the stash, a fifth when the chunk starts between two, funnel-shifted and byte-swapped; the record's length is read once per
// chunk, not once per word: 2.8 -> 2.3 ms per 2*10^7 strands of 100 bases in rows scattered by the sorted job); the chunk that holds the sequence's last
// bytes, and rows too short for a whole chunk, go word by word as before.  Same conditions under which a record describes a complete
// sequence (k_ovl_walk: not empty, not longer than max_len, longer than min_match unless info_only).  Bytes of a row beyond the sequence
// are written only inside the word that holds its last base (zeros), as before.
__device__ __forceinline__ void seq_out_word(const uint8_t *sr, int L, uint32_t w, uint8_t *dst)
{
    // output bytes 4w..4w+3 = stash bytes a+3..a with a = L - 4 - 4w: an unaligned word, byte-swapped
    const int a = L - 4 - (int)(4 * w);
    uint32_t v;
    if (a >= 0) {
        const uint32_t *q = (const uint32_t *)(sr + (a & ~3));
        const uint64_t two = (a & 3) ? ((uint64_t)q[1] << 32 | q[0]) : q[0];
        v = __builtin_bswap32((uint32_t)(two >> (8 * (a & 3))));
    } else v = __builtin_bswap32(*(const uint32_t *)sr << (8 * -a)); // the first 4 + a bases of the stash, the rest of the word zero
    *(uint32_t *)(dst + 4 * w) = v;
}
__global__ void k_ovl_seq_out(size_t n, uint32_t chunks, const uint8_t *__restrict__ srev, uint32_t stride_r, const fmd_ovlp_rec_t *__restrict__ rec,
                              int min_match, int info_only, uint8_t *__restrict__ seq_out, uint32_t seq_stride, const uint32_t *__restrict__ gidx)
{
    const size_t total = n * (size_t)chunks, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const size_t sid = i / chunks;
        const uint32_t c = (uint32_t)(i - sid * chunks), o = 16 * c;
        const size_t g = gidx ? (size_t)gidx[sid] : sid;   // the strand's row in rec[] and seq_out[] (sorted batches: fmd_ovlp_sorted_dev)
        const int L = rec[g].len;
        if (L <= 0 || (uint32_t)L > stride_r || (!info_only && L <= min_match) || (int)o >= L) continue;
        const uint8_t *sr = srev + sid * (size_t)stride_r;
        uint8_t *dst = seq_out + g * (size_t)seq_stride;
        if ((int)o + 16 <= L && o + 16 <= seq_stride) {   // a whole chunk inside the sequence: stash bytes [a, a + 16), a >= 0
            const int a = L - 16 - (int)o;
            const uint32_t sh = 8 * ((uint32_t)a & 3);
            const uint32_t *q = (const uint32_t *)(sr + (a & ~3));
            const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = sh ? q[4] : 0u;   // (q[4] holds stash bytes below a + 16 <= L: inside the row)
            const uint32_t d0 = sh ? (uint32_t)(((uint64_t)q1 << 32 | q0) >> sh) : q0, d1 = sh ? (uint32_t)(((uint64_t)q2 << 32 | q1) >> sh) : q1;
            const uint32_t d2 = sh ? (uint32_t)(((uint64_t)q3 << 32 | q2) >> sh) : q2, d3 = sh ? (uint32_t)(((uint64_t)q4 << 32 | q3) >> sh) : q3;
            uint32_t *out = (uint32_t *)(dst + o);
            out[0] = __builtin_bswap32(d3); out[1] = __builtin_bswap32(d2); out[2] = __builtin_bswap32(d1); out[3] = __builtin_bswap32(d0);
        } else {
#pragma unroll
            for (uint32_t w = 4 * c; w < 4 * c + 4; ++w)
                if ((int)(4 * w) < L && 4 * w + 3 < seq_stride) seq_out_word(sr, L, w, dst);
        }
    }
}

// What WALK_HEAD needs to take a strand in, resolved for every strand beforehand by a streaming kernel (one thread per strand) instead
// of a chain of four dependent loads in front of a wave's gather: item t of the head's order -> its row, and where its walk stands
// behind the tail table (FmdIndexView::tail + two prefix-table entries; the items come sorted by tail, so neighbouring threads read
// neighbouring entries).  32 bytes per strand:
//   a = { row, k lo, x0 lo, x1 lo }   b = { size lo, k hi | x0 hi << 8 | x1 hi << 16 | size hi << 24, tail as a prefix-table index, flags }
// flags bit 0: no tail-table entry (shorter than ptab_d bases, or a base that is not A/C/G/T among them): k = the sequence id, and
// the walk starts at its sentinel.
__global__ void k_ovl_head_adm(FmdIndexView ix, size_t n, const uint64_t *__restrict__ ids, const uint32_t *__restrict__ order, int use_tail,
                               uint4 *__restrict__ adm)
{
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += step) {
        const uint32_t row = order ? order[t] : (uint32_t)t;
        const uint64_t id = ids[row];
        const unsigned long long te = (use_tail && id < ix.n_seq) ? ix.tail[id] : ~0ull;
        uint4 a, b;
        if (te != ~0ull) {
            const uint32_t tfw = (uint32_t)(te >> (64 - 2 * ix.ptab_d));
            const uint64_t k = te & ((1ull << (64 - 2 * ix.ptab_d)) - 1);
            uint32_t r = __brev(~tfw) >> (32 - 2 * ix.ptab_d);   // reverse complement of the ptab index: the 2-bit groups in reverse order, complemented
            const uint32_t trv = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
            const uint4 ef = ix.ptab[tfw], er = ix.ptab[trv];
            fmd_count_lane(ix, 2, 1);
            const uint64_t x0 = (uint64_t)ef.y << 32 | ef.x, sz = ((uint64_t)ef.w << 32 | ef.z) - x0 + 1, x1 = (uint64_t)er.y << 32 | er.x;
            a = make_uint4(row, (uint32_t)k, (uint32_t)x0, (uint32_t)x1);
            b = make_uint4((uint32_t)sz, (uint32_t)(k >> 32) | (uint32_t)(x0 >> 32) << 8 | (uint32_t)(x1 >> 32) << 16 | (uint32_t)(sz >> 32) << 24, tfw, 0u);
        } else {
            a = make_uint4(row, (uint32_t)id, 0u, 0u);
            b = make_uint4(0u, (uint32_t)(id >> 32) & 0xffu, 0u, 1u);
        }
        adm[2 * t] = a; adm[2 * t + 1] = b;
    }
}

// ------------------------------------------------------------------------------- launchers
// tickets per atomic of a walk launch (FmdTickets::chunk): `dflt` for large launches, never more than a 64th of a wave's share
// (the last chunks of a launch are worked off by fewer and fewer waves)
static uint32_t walk_ticket_chunk(uint32_t dflt, size_t n, int grid)
{
    const size_t share = n / (size_t)(grid > 0 ? grid : 1) / 64;
    const uint32_t c = dflt > share ? (uint32_t)share : dflt;
    return c < FMD_TICKET_CHUNK ? FMD_TICKET_CHUNK : c;
}
// waves of a walk launch: what the CUs hold at lds_bytes each, at most per_cu per CU where the caller leaves room for another phase (FMD_OVLP_PIPE)
static int walk_grid(const fmd_dev *h, size_t n, size_t lds_bytes, int per_cu)
{
    const int grid = fmd_grid_for_lds(h, n, lds_bytes);
    return per_cu > 0 && grid > h->n_cu * per_cu ? h->n_cu * per_cu : grid;
}
static void launch_seq_out(hipStream_t st, size_t n, uint32_t max_len, const uint8_t *srev, uint32_t stride_r, const fmd_ovlp_rec_t *rec, int min_match,
                           int info_only, uint8_t *seq_out, uint32_t seq_stride, const uint32_t *gidx)
{
    const uint32_t chunks = (max_len + 15) / 16;
    const size_t total = n * (size_t)chunks;
    size_t blocks = (total + 255) / 256;
    if (blocks > (1u << 22)) blocks = 1u << 22;
    k_ovl_seq_out<<<(unsigned)blocks, 256, 0, st>>>(n, chunks, srev, stride_r, rec, min_match, info_only, seq_out, seq_stride, gidx);
}

void fmd_launch_walk_whole(fmd_dev *h, hipStream_t st, WalkArgs a, uint32_t max_len, uint8_t *seq_out, uint32_t seq_stride, int per_cu, uint32_t tickets)
{
    const int grid = walk_grid(h, a.n, FMD_COMPACT_LDS_U4 * 16, per_cu);
    a.queue = fmd_next_queue(h, st); a.tickets = walk_ticket_chunk(tickets, a.n, grid);
    k_ovl_walk<WALK_WHOLE><<<grid, 64, 0, st>>>(a);
    launch_seq_out(st, a.n, max_len, a.srev, a.stride_r, a.rec, a.min_match, a.info_only, seq_out, seq_stride, nullptr);
}
void fmd_launch_walk_tail(fmd_dev *h, hipStream_t st, WalkArgs a, uint32_t max_len, uint8_t *seq_out, uint32_t seq_stride, int per_cu)
{
    const int grid = walk_grid(h, a.n, FMD_COMPACT_LDS_U4 * 16, per_cu);
    a.queue = fmd_next_queue(h, st); a.tickets = walk_ticket_chunk(64, a.n, grid);
    k_ovl_walk<WALK_TAIL><<<grid, 64, 0, st>>>(a);
    launch_seq_out(st, a.n, max_len, a.srev, a.stride_r, a.rec, a.min_match, 0, seq_out, seq_stride, a.gidx);
}
bool fmd_walk_tail2_fits(uint32_t stride_r, uint32_t seq_stride) { return stride_r <= WALK_LS_BASES && seq_stride >= stride_r + 4 && (seq_stride & 3) == 0; }
void fmd_launch_walk_tail2(fmd_dev *h, hipStream_t st, WalkArgs a, int per_cu)
{
    const int grid = walk_grid(h, a.n, FMD_COMPACT_LDS_U4 * 16 + 64 * WALK_LS_WORDS * 4, per_cu);
    a.queue = fmd_next_queue(h, st); a.tickets = a.keys ? 64u : walk_ticket_chunk(64, a.n, grid);   // (in phase: one chunk = one generation of a wave)
    (void)hipMemsetAsync(a.redo, 0, 4, st);
    if (a.cls) (void)hipMemsetAsync(a.cls, 0, 4 * FMD_CLS_HEADER_U32, st);
    k_ovl_walk<WALK_TAIL2><<<grid, 64, 0, st>>>(a);
    k_ovl_seq_redo<<<64, 64, 0, st>>>(a.ix, a.redo, a.gidx, a.park, a.rec, a.seq_out, a.seq_stride);
}

int fmd_ovlp_head(fmd_dev *h, hipStream_t st, size_t n, const uint64_t *d_ids, int min_match, fmd_ovlp_rec_t *d_rec, FmdWalkPark *park,
                  uint32_t *keys_a, uint32_t *vals_a, uint32_t *keys_sorted, uint32_t *order, void *tmp, size_t tmp_bytes, uint4 *adm)
{
    (void)fmd_pairs_ensure(h, 0);          // the two-base blocks: built here only where FMD_PAIR asks for it (fmd_pair.hip); a caller that keeps the index for many passes calls fmd_dev_build_pairs
    const FmdIndexView ix = fmd_view(h);
    // pass 1: every strand FMD_WALK_SPLIT bases in, in the caller's order.  (Taking the strands in the order of their last ptab_d bases --
    // the tail table has them, one more radix sort -- makes this pass 7 % faster and costs what it saves: profiles/r3_locality.)
    {
        const uint32_t *order1 = nullptr;
        const int use_tail = ix.tail != nullptr && ix.ptab != nullptr && min_match >= ix.ptab_d && ix.ptab_d >= 2;
        size_t blocks = (n + 255) / 256;
        if (blocks > (1u << 20)) blocks = 1u << 20;
        k_ovl_head_adm<<<(unsigned)blocks, 256, 0, st>>>(ix, n, d_ids, order1, use_tail, adm);
        const int grid = fmd_grid_for_lds(h, n, FMD_COMPACT_LDS_U4 * 16);
        WalkArgs a;   // what every launch of the head takes; the items, their admission records and the hand-over depth differ
        a.ix = ix; a.ids = d_ids; a.min_match = min_match; a.rec = d_rec; a.park = park;
        a.stride_r = (uint32_t)sizeof(FmdWalkPark);   // (no sequence that ends inside the head is longer)
        a.n = n; a.adm = adm; a.queue = fmd_next_queue(h, st); a.tickets = walk_ticket_chunk(256, n, grid);
        bool pairs = ix.pair != nullptr && ix.pair_tab != nullptr && n >= 4096 && n < 0xffffff00ull;
        { const char *e = getenv("FMD_PAIR_USE"); if (e && atoi(e) == 0) pairs = false; }   // A/B switch on a handle that has the blocks
        FmdScratch strag_l, adm2_l;
        if (pairs) strag_l.alloc(h, (n + 1) * 4);
        uint32_t *strag = strag_l.as<uint32_t>();
        if (strag) {
            // single steps up to `from` (by then a strand's interval is narrow), two bases per request from there to FMD_WALK_SPLIT (k_ovl_pair), and
            // the strands that kernel could not take all the way once more from their admission records, single steps all the way
            int from = 16;
            { const char *e = getenv("FMD_PAIR_FROM"); if (e && atoi(e) > ix.ptab_d && atoi(e) < (int)FMD_WALK_SPLIT && !(atoi(e) & 1)) from = atoi(e); }
            if (from <= ix.ptab_d) from = (ix.ptab_d + 2) & ~1;
            a.pair_from = from;
            k_ovl_walk<WALK_HEAD><<<grid, 64, 0, st>>>(a);
            (void)hipMemsetAsync(strag, 0, 4, st);
            uint32_t *q2 = fmd_next_queue(h, st);
            int grid2 = h->n_cu * (FMD_PAIR_LB * 4 < 20 ? FMD_PAIR_LB * 4 : 20);      // (8 KiB of LDS per wave: twenty fit a CU)
            if ((size_t)grid2 > (n + 63) / 64) grid2 = (int)((n + 63) / 64);
            k_ovl_pair<<<grid2, 64, 0, st>>>(ix, n, park, q2, walk_ticket_chunk(256, n, grid2), strag);
            uint32_t n_strag = 0;
            hipError_t e1 = hipMemcpyAsync(&n_strag, strag, 4, hipMemcpyDeviceToHost, st);
            if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);
            if (e1 != hipSuccess) { fmd_set_hip_error(e1, "two-base pass"); return FMD_E_HIP; }
            if (n_strag) {
                if (adm2_l.alloc(h, (size_t)n_strag * 32)) return FMD_E_NOMEM;
                uint4 *adm2 = adm2_l.as<uint4>();
                k_ovl_strag_adm<<<(n_strag + 255) / 256 < 65536 ? (n_strag + 255) / 256 : 65536, 256, 0, st>>>(strag, adm, adm2);
                const int grid3 = fmd_grid_for_lds(h, n_strag, FMD_COMPACT_LDS_U4 * 16);
                a.n = n_strag; a.adm = adm2; a.pair_from = 0; a.queue = fmd_next_queue(h, st); a.tickets = walk_ticket_chunk(256, n_strag, grid3);
                k_ovl_walk<WALK_HEAD><<<grid3, 64, 0, st>>>(a);
                e1 = hipStreamSynchronize(st);      // (adm2 goes back to the handle's cache)
                adm2_l.reset();
                if (e1 != hipSuccess) { fmd_set_hip_error(e1, "two-base pass"); return FMD_E_HIP; }
            }
            strag_l.reset();
            if (getenv("FMD_DEBUG_PAIR")) fprintf(stderr, "[M::ovl_head] two-base pass from depth %d: %u of %zu strands walked again one base at a time\n", from, n_strag, n);
        } else k_ovl_walk<WALK_HEAD><<<grid, 64, 0, st>>>(a);
    }
    // the order of pass 2: rows sorted by the minimizer of the bases each strand has shown so far
    return fmd_park_sort(st, n, park, keys_a, keys_sorted, vals_a, order, tmp, tmp_bytes);
}
