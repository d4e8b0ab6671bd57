// fmd_ovlp_nei.hip -- overlap discovery, one lane per strand with the candidate lists in HBM: fm6_get_nei for the strands the group kernels
// set aside or hand back (k_ovl_nei), the fake-fork fix-up on its own (k_ovl_fix), check_left_simple (k_ovl_cls), and their launchers.
#include "fmd_ovlp_internal.h"

// --------------------------------------------------------------------- phase B: fm6_get_nei
// unitig.c:93-179.  Latency is the enemy here (three dependent rank2a per candidate interval), so
// nothing but the rank fetch is allowed on a wave step's critical path:
//   * the next candidate interval is prefetched into registers while the current one is extended
//     (its load completes under the same s_waitcnt as the rank-block gather);
//   * the first child pushed in a round and the first neighbour stay in registers;
//   * categories (unitig.c:143-151) are assigned while pushing, because children are pushed in
//     sorted order unless a category forks; the stored entry keeps the original sort key in the
//     spare top 16 bits of its size word, and only a round that saw an out-of-order push takes
//     the slow path (sort + recompute), exactly as ks_introsort + the recompute loop would.
enum { ST_IDLE = 0, ST_PICK, ST_EXT, ST_E0, ST_C, ST_FIX1, ST_FIX2 };

struct I3 { uint64_t x0, x1, sz; };
// field-wise select (keeps the candidates in registers; a struct ternary chain goes through scratch)
__device__ __forceinline__ I3 pick5(int c, const I3 &a0, const I3 &a1, const I3 &a2, const I3 &a3, const I3 &a4)
{
    I3 r;
    r.x0 = sel6(c, a0.x0, a1.x0, a2.x0, a3.x0, a4.x0, a0.x0);
    r.x1 = sel6(c, a0.x1, a1.x1, a2.x1, a3.x1, a4.x1, a0.x1);
    r.sz = sel6(c, a0.sz, a1.sz, a2.sz, a3.sz, a4.sz, a0.sz);
    return r;
}


__global__ __launch_bounds__(64) void k_ovl_nei(FmdIndexView ix, size_t n, int min_match, const uint8_t *__restrict__ srev,
                                                uint32_t stride_r, uint32_t cap, fmd_intv_t *__restrict__ listA,
                                                fmd_intv_t *__restrict__ listB, fmd_ovlp_rec_t *__restrict__ rec,
                                                fmd_intv_t *__restrict__ nei_out, uint32_t max_nei,
                                                uint8_t *__restrict__ seq_out, uint32_t seq_stride, uint32_t *__restrict__ queue,
                                                const uint32_t *__restrict__ work_list, const uint32_t *__restrict__ work_n,
                                                const uint32_t *__restrict__ gidx)
{
    FMD_DECLARE_WAVE_LDS();
    if (work_list) n = *work_n;   // only the strands the group kernels could not take
    // per-lane search state
    size_t sid = 0;   // the strand's slot in the batch (rows of srev, listA, listB)
    size_t gs = 0;    // its row in rec[], nei_out[], seq_out[] (gidx[sid] in a sorted batch, sid otherwise)
    int st = ST_IDLE, ori_l = 0, cur_l = 0, cpend = 0, first_c = 0, masked_cat = -2, cat_j = 0, fix_i = 0;
    uint32_t prev_n = 0, curr_n = 0, j = 0, n_nei = 0, flags = 0, cat0 = 0, last_hi = 0;
    bool unsorted = false, exhausted = false, prev_is_a = true, e_valid = false;
    fmd_intv_t *prev = nullptr, *curr = nullptr;
    uint64_t last_key = 0;
    uint4 ea = make_uint4(0, 0, 0, 0), eb = make_uint4(0, 0, 0, 0); // prefetched prev[j], raw (decoded at pick time)
    uint64_t fx0 = 0, fx1 = 0, fsz = 0, finfo = 0;   // first child pushed this round (= next round's prev[0])
    uint64_t px0 = 0, px1 = 0, psz = 0, pinfo = 0;   // interval being extended
    I3 o0 = {0, 0, 0}, oc1 = {0, 0, 0}, oc2 = {0, 0, 0}, oc3 = {0, 0, 0}, oc4 = {0, 0, 0}; // its children
    uint64_t nx0 = 0, nsz = 0, ninfo = 0;             // first neighbour

    FmdTickets tk_;
    fmd_tickets_init(tk_, queue);
    for (;;) {
        // ---- refill
        const size_t my = fmd_tickets_take(tk_, queue, st == ST_IDLE && !exhausted);
        if (st == ST_IDLE && !exhausted) {
            if (my < n) {
                const size_t strand = work_list ? (size_t)work_list[my] : my;
                const size_t grow = gidx ? (size_t)gidx[strand] : strand;
                const fmd_ovlp_rec_t *o = rec + grow;
                if (o->status == 0 && o->n_ovlp > 0 && !(o->flags & FMD_OVLP_F_OVERFLOW)) {
                    sid = strand; gs = grow; ori_l = cur_l = o->len;
                    prev_n = (uint32_t)o->n_ovlp; curr_n = 0; j = 0;
                    prev = listA + sid * (size_t)cap + (cap - prev_n);
                    curr = listB + sid * (size_t)cap; prev_is_a = true;
                    n_nei = 0; flags = 0; masked_cat = -2; unsorted = false; last_key = 0; cat0 = 0;
                    e_valid = false;
                    st = ST_PICK;
                }
            } else exhausted = true;
        }
        // ---- bookkeeping that needs no rank: pick the next interval / finish a round / finish
        while (st == ST_PICK) {
            if (j < prev_n) {
                if (!e_valid) { const uint4 *q = (const uint4 *)(prev + j); ea = q[0]; eb = q[1]; }
                if (cur_l == ori_l) { // round 0: the walk's candidates (either form); it stored the suffix depth, unitig.c:53 wants the start
                    const FmdCand cd = cand_decode(ea, eb);
                    cat_j = 0;
                    px0 = cd.x0; px1 = cd.x1; psz = cd.sz; pinfo = (uint64_t)ori_l - cd.depth;
                } else {
                    cat_j = (int)(eb.w >> 4);                    // info >> 36
                    px0 = (uint64_t)ea.y << 32 | ea.x; px1 = (uint64_t)ea.w << 32 | ea.z;
                    psz = ((uint64_t)eb.y << 32 | eb.x) & FMD_SZ_MASK; pinfo = (uint64_t)eb.w << 32 | eb.z;
                }
                if (cat_j == masked_cat) { ++j; e_valid = false; continue; }
                st = ST_EXT;
                e_valid = j + 1 < prev_n;
                if (e_valid) { const uint4 *q = (const uint4 *)(prev + j + 1); ea = q[0]; eb = q[1]; } // lands under the rank fetch
            } else if (curr_n) { // end of a round (unitig.c:137-153)
                if ((uint32_t)cur_l < seq_stride) seq_out[gs * (size_t)seq_stride + cur_l] = (uint8_t)comp6(first_c);
                ++cur_l;
                if (unsorted) { // slow path: ks_introsort by the original keys, then recompute the categories
                    for (uint32_t a = 1; a < curr_n; ++a) {
                        uint64_t ax0, ax1, asz, ainf;
                        load_entry(curr + a, ax0, ax1, asz, ainf);
                        const uint64_t akey = (asz >> 48) << 32 | (ainf & 0xffffffffull);
                        uint32_t b = a;
                        while (b > 0) {
                            uint64_t bx0, bx1, bsz, binf;
                            load_entry(curr + b - 1, bx0, bx1, bsz, binf);
                            if (((bsz >> 48) << 32 | (binf & 0xffffffffull)) <= akey) break;
                            store_entry(curr + b, bx0, bx1, bsz, binf);
                            --b;
                        }
                        store_entry(curr + b, ax0, ax1, asz, ainf);
                    }
                    uint32_t last = 0; cat0 = 0;
                    for (uint32_t a = 0; a < curr_n; ++a) {
                        uint64_t ax0, ax1, asz, ainf;
                        load_entry(curr + a, ax0, ax1, asz, ainf);
                        const uint32_t hi = (uint32_t)(asz >> 48);
                        if (a == 0) last = hi; else if (hi != last) { last = hi; cat0 = a; }
                        ainf = (ainf & 0xffffffffull) | (uint64_t)cat0 << 36;
                        curr[a].info = ainf;
                        if (a == 0) { fx0 = ax0; fx1 = ax1; fsz = asz & FMD_SZ_MASK; finfo = ainf; }
                    }
                }
                if (cat0 != 0) flags |= FMD_OVLP_F_FORKED;
                prev_is_a = !prev_is_a; // both lists start at index 0 of their areas from now on
                prev = (prev_is_a ? listA : listB) + sid * (size_t)cap;
                curr = (prev_is_a ? listB : listA) + sid * (size_t)cap;
                prev_n = curr_n; curr_n = 0; j = 0; masked_cat = -2; unsorted = false; last_key = 0; cat0 = 0;
                ea = make_uint4((uint32_t)fx0, (uint32_t)(fx0 >> 32), (uint32_t)fx1, (uint32_t)(fx1 >> 32));
                eb = make_uint4((uint32_t)fsz, (uint32_t)(fsz >> 32), (uint32_t)finfo, (uint32_t)(finfo >> 32)); e_valid = true;
            } else { // all paths closed (unitig.c:154-178)
                fmd_ovlp_rec_t *o = rec + gs;
                const int rbeg = ori_l - (int)(uint32_t)ninfo;
                if (n_nei == 1 && (flags & FMD_OVLP_F_FORKED) && !(flags & FMD_OVLP_F_FIXED) && rbeg < ori_l) {
                    // contained reads made a fake fork: re-derive the appended bases (unitig.c:158-176)
                    o0.x0 = 0; o0.x1 = 0; o0.sz = ix.cnt[1]; // fm6_set_intv(e, 0, ok0)
                    fix_i = rbeg;
                    st = ST_FIX1;
                    break;
                }
                if (n_nei > 1) cur_l = ori_l;
                o->rbeg = n_nei ? rbeg : -1;
                o->ext_len = cur_l - ori_l; o->n_nei = (int32_t)n_nei; o->flags |= flags;
                st = ST_IDLE;
            }
        }
        if (__ballot(st != ST_IDLE) == 0) { if (__ballot(!exhausted) == 0) break; else continue; }

        // ---- one rank2a request per lane
        uint64_t qk = NONE64, ql = NONE64;
        if (st == ST_EXT) { qk = px1 - 1; ql = px1 - 1 + psz; }                    // forward: strand x[1]
        else if (st == ST_E0) { qk = o0.x0 - 1; ql = o0.x0 - 1 + o0.sz; }          // backward: strand x[0]
        else if (st == ST_C) {
            const uint64_t a = cpend == 1 ? oc1.x0 : cpend == 2 ? oc2.x0 : cpend == 3 ? oc3.x0 : oc4.x0;
            const uint64_t z = cpend == 1 ? oc1.sz : cpend == 2 ? oc2.sz : cpend == 3 ? oc3.sz : oc4.sz;
            qk = a - 1; ql = a - 1 + z;
        } else if (st == ST_FIX1 || st == ST_FIX2) { qk = o0.x1 - 1; ql = o0.x1 - 1 + o0.sz; }
        const FmdRank2 r = fmd_wave_rank2_fetch(ix, fmd_lds, qk, ql);

        // ---- consume
        if (st == ST_EXT || st == ST_FIX1 || st == ST_FIX2) {
            uint64_t tk[6] = {0, 0, 0, 0, 0, 0}, tl[6] = {0, 0, 0, 0, 0, 0};
            if (r.hk) fmd_block_rank6<false>(r.bk, r.t, r.nk, tk, r.blk_k);
            if (r.hl) fmd_block_rank6<false>(r.bl, r.tl, r.nl, tl, r.blk_l);
            uint64_t s[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) s[c] = tl[c] - tk[c];
            // forward extension (exact.c:72-88, is_back = 0): x[1] from rank, x[0] running sum
            const uint64_t base0 = st == ST_EXT ? px0 : o0.x0;
            I3 k0, k1, k2, k3, k4;
            k0.x0 = base0;            k0.x1 = ix.cnt[0] + tk[0]; k0.sz = s[0];
            k4.x0 = k0.x0 + s[0];     k4.x1 = ix.cnt[4] + tk[4]; k4.sz = s[4];
            k3.x0 = k4.x0 + s[4];     k3.x1 = ix.cnt[3] + tk[3]; k3.sz = s[3];
            k2.x0 = k3.x0 + s[3];     k2.x1 = ix.cnt[2] + tk[2]; k2.sz = s[2];
            k1.x0 = k2.x0 + s[2];     k1.x1 = ix.cnt[1] + tk[1]; k1.sz = s[1];
            if (st == ST_EXT) {
                o0 = k0; oc1 = k1; oc2 = k2; oc3 = k3; oc4 = k4;
                if (o0.sz && cur_l != ori_l) st = ST_E0;   // some reads end here (unitig.c:111)
                else {
                    cpend = oc1.sz ? 1 : oc2.sz ? 2 : oc3.sz ? 3 : oc4.sz ? 4 : 0;
                    if (cpend) st = ST_C; else { ++j; st = ST_PICK; }
                }
            } else if (st == ST_FIX1) { // unitig.c:160-163
                const int b = seq_out[gs * (size_t)seq_stride + fix_i];   // (the caller's row holds the sequence in read order by now: the stash is the walk's own)
                const int c = comp6(b);
                o0 = pick5(c, k0, k1, k2, k3, k4);
                if (c == 5) { o0.x0 = k1.x0 + s[1]; o0.x1 = ix.cnt[5] + tk[5]; o0.sz = s[5]; }
                ++fix_i;
                if (fix_i == ori_l) { st = ori_l < cur_l ? ST_FIX2 : ST_PICK; flags |= FMD_OVLP_F_FIXED; }
            } else { // ST_FIX2: unitig.c:164-175
                int cnt_ok = 0, c0 = -1;
#define FMD_FIX_TRY(c, kc) if (kc.sz && kc.x0 <= nx0 && kc.x0 + kc.sz >= nx0 + nsz) { ++cnt_ok; c0 = c; }
                FMD_FIX_TRY(1, k1) FMD_FIX_TRY(2, k2) FMD_FIX_TRY(3, k3) FMD_FIX_TRY(4, k4)
#undef FMD_FIX_TRY
                bool stop = (cnt_ok == 0 && k0.sz != 0);
                if (!stop && c0 > 0) {
                    if ((uint32_t)fix_i < seq_stride) seq_out[gs * (size_t)seq_stride + fix_i] = (uint8_t)comp6(c0);
                    o0 = pick5(c0, k0, k1, k2, k3, k4);
                    ++fix_i;
                    if (fix_i == cur_l) stop = true;
                } else stop = true;
                if (stop) { cur_l = fix_i; st = ST_PICK; }
            }
        } else if (st == ST_E0 || st == ST_C) {
            // fm6_extend0 (exact.c:90-98), backward: only the '$' child matters
            const uint64_t t0k = r.hk ? fmd_block_rank1(r.bk, r.t, r.nk, 0, r.blk_k) : 0;
            const uint64_t t0l = r.hl ? fmd_block_rank1(r.bl, r.tl, r.nl, 0, r.blk_l) : 0;
            const uint64_t e0sz = t0l - t0k;
            if (st == ST_E0) {
                bool is_nei = false;
                if (e0sz && o0.sz == psz && psz == e0sz) { // bounded by sentinels on both sides and not contained
                    const uint64_t inf = (uint64_t)ori_l - (pinfo & 0xffffffffull);
                    if (n_nei == 0) { nx0 = t0k; nsz = e0sz; ninfo = inf; }
                    if (n_nei < max_nei) store_entry(nei_out + gs * (size_t)max_nei + n_nei, t0k, o0.x1, e0sz, inf);
                    else flags |= FMD_OVLP_F_OVERFLOW;
                    ++n_nei;
                    masked_cat = cat_j; // mask out the other intervals of this category
                    is_nei = true;
                }
                if (is_nei) { ++j; st = ST_PICK; }
                else {
                    cpend = oc1.sz ? 1 : oc2.sz ? 2 : oc3.sz ? 3 : oc4.sz ? 4 : 0;
                    if (cpend) st = ST_C; else { ++j; st = ST_PICK; }
                }
            } else {
                if (e0sz) { // left end bounded by a sentinel: keep the child (unitig.c:128-135)
                    const I3 ch = pick5(cpend, oc1, oc1, oc2, oc3, oc4);
                    const uint64_t key = (pinfo & 0xfffffff0ffffffffull) | (uint64_t)cpend << 32;
                    const uint32_t hi = (uint32_t)(key >> 32);  // old category << 4 | base
                    if (curr_n < cap) {
                        if (curr_n == 0) { first_c = cpend; cat0 = 0; last_hi = hi; }
                        else {
                            if (key < last_key) unsorted = true;
                            if (hi != last_hi) { cat0 = curr_n; last_hi = hi; }
                        }
                        last_key = key;
                        const uint64_t inf = (key & 0xffffffffull) | (uint64_t)cat0 << 36;
                        store_entry(curr + curr_n, ch.x0, ch.x1, ch.sz | (uint64_t)hi << 48, inf);
                        if (curr_n == 0) { fx0 = ch.x0; fx1 = ch.x1; fsz = ch.sz; finfo = inf; }
                        ++curr_n;
                    } else { flags |= FMD_OVLP_F_OVERFLOW; }
                }
                int nc = 0;
                if (cpend < 2 && oc2.sz) nc = 2; else if (cpend < 3 && oc3.sz) nc = 3; else if (cpend < 4 && oc4.sz) nc = 4;
                if (nc) cpend = nc; else { ++j; st = ST_PICK; }
            }
        }
        // an overflowing strand is abandoned; the host re-runs it with larger capacities
        if (st != ST_IDLE && (flags & FMD_OVLP_F_OVERFLOW)) {
            fmd_ovlp_rec_t *o = rec + gs;
            o->flags |= FMD_OVLP_F_OVERFLOW; o->n_nei = 0; o->rbeg = -1; o->ext_len = 0;
            st = ST_IDLE;
        }
    }
}

// ------------------------------------------------------------ the fake-fork fix-up on its own
// unitig.c:158-176 for strands the group kernels closed with ONE neighbour after a fork (contained reads made the fork): the record,
// the neighbour and the appended bases are there as fm6_get_nei's loop leaves them; what remains is to walk the overlap string
// forward from the empty interval (FIX1: ori_l - rbeg dependent steps) and then re-derive the appended bases as long as exactly one
// child still contains the neighbour's interval (FIX2).  k_ovl_nei does the same at the end of its own pass -- after redoing the
// whole of fm6_get_nei with lists in HBM, which is what this kernel spares the strands the group kernels had finished.
__global__ __launch_bounds__(64) void k_ovl_fix(FmdIndexView ix, const uint32_t *__restrict__ list, const uint32_t *__restrict__ list_n,
                                                const uint8_t *__restrict__ srev, uint32_t stride_r, fmd_ovlp_rec_t *__restrict__ rec,
                                                const fmd_intv_t *__restrict__ nei_out, uint32_t max_nei, uint8_t *__restrict__ seq_out, uint32_t seq_stride,
                                                uint32_t *__restrict__ queue, const uint32_t *__restrict__ gidx)
{
    FMD_DECLARE_WAVE_LDS();
    const size_t n = *list_n;
    size_t sid = 0, gs = 0;
    int st = 0, ori_l = 0, cur_l = 0, fix_i = 0;   // st: 0 idle, 1 = FIX1, 2 = FIX2
    uint64_t x0 = 0, x1 = 0, sz = 0, nx0 = 0, nsz = 0;
    bool exhausted = false;
    FmdTickets tk_;
    fmd_tickets_init(tk_, queue);
    for (;;) {
        const size_t my = fmd_tickets_take(tk_, queue, st == 0 && !exhausted);
        if (st == 0 && !exhausted) {
            if (my < n) {
                sid = list[my]; gs = gidx ? (size_t)gidx[sid] : sid;
                const fmd_ovlp_rec_t *o = rec + gs;
                ori_l = o->len; cur_l = ori_l + o->ext_len; fix_i = o->rbeg;
                const uint4 *q = (const uint4 *)(nei_out + gs * (size_t)max_nei);
                const uint4 a = q[0], b = q[1];
                nx0 = (uint64_t)a.y << 32 | a.x; nsz = (uint64_t)b.y << 32 | b.x;
                x0 = 0; x1 = 0; sz = ix.cnt[1];                      // fm6_set_intv(e, 0, ok0)
                if (fix_i >= 0 && fix_i < ori_l) st = 1;
            } else exhausted = true;
        }
        if (__ballot(st != 0) == 0) { if (__ballot(!exhausted) == 0) break; else continue; }
        const FmdRank2 r = fmd_wave_rank2_fetch(ix, fmd_lds, st ? x1 - 1 : NONE64, st ? x1 - 1 + sz : NONE64);   // forward: strand x[1]
        if (st == 0) continue;
        uint64_t tk[6] = {0, 0, 0, 0, 0, 0}, tl[6] = {0, 0, 0, 0, 0, 0}, s[6];
        if (r.hk) fmd_block_rank6<false>(r.bk, r.t, r.nk, tk, r.blk_k);
        if (r.hl) fmd_block_rank6<false>(r.bl, r.tl, r.nl, tl, r.blk_l);
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] = tl[c] - tk[c];
        // forward extension (exact.c:72-88, is_back = 0): x[1] from rank, x[0] running sum in the order $, T, G, C, A, N
        I3 k0, k1, k2, k3, k4;
        k0.x0 = x0;               k0.x1 = ix.cnt[0] + tk[0]; k0.sz = s[0];
        k4.x0 = k0.x0 + s[0];     k4.x1 = ix.cnt[4] + tk[4]; k4.sz = s[4];
        k3.x0 = k4.x0 + s[4];     k3.x1 = ix.cnt[3] + tk[3]; k3.sz = s[3];
        k2.x0 = k3.x0 + s[3];     k2.x1 = ix.cnt[2] + tk[2]; k2.sz = s[2];
        k1.x0 = k2.x0 + s[2];     k1.x1 = ix.cnt[1] + tk[1]; k1.sz = s[1];
        bool done = false;
        if (st == 1) { // unitig.c:160-163
            const int b = seq_out[gs * (size_t)seq_stride + fix_i];
            const int c = comp6(b);
            I3 n3 = pick5(c, k0, k1, k2, k3, k4);
            if (c == 5) { n3.x0 = k1.x0 + s[1]; n3.x1 = ix.cnt[5] + tk[5]; n3.sz = s[5]; }
            x0 = n3.x0; x1 = n3.x1; sz = n3.sz;
            ++fix_i;
            if (fix_i == ori_l) { if (ori_l < cur_l) st = 2; else done = true; }
        } else {       // unitig.c:164-175
            int cnt_ok = 0, c0 = -1;
#define FMD_FIX_TRY(c, kc) if (kc.sz && kc.x0 <= nx0 && kc.x0 + kc.sz >= nx0 + nsz) { ++cnt_ok; c0 = c; }
            FMD_FIX_TRY(1, k1) FMD_FIX_TRY(2, k2) FMD_FIX_TRY(3, k3) FMD_FIX_TRY(4, k4)
#undef FMD_FIX_TRY
            bool stop = (cnt_ok == 0 && k0.sz != 0);
            if (!stop && c0 > 0) {
                if ((uint32_t)fix_i < seq_stride) seq_out[gs * (size_t)seq_stride + fix_i] = (uint8_t)comp6(c0);
                const I3 n3 = pick5(c0, k0, k1, k2, k3, k4);
                x0 = n3.x0; x1 = n3.x1; sz = n3.sz;
                ++fix_i;
                if (fix_i == cur_l) stop = true;
            } else stop = true;
            if (stop) { cur_l = fix_i; done = true; }
        }
        if (done) {
            fmd_ovlp_rec_t *o = rec + gs;
            o->ext_len = cur_l - ori_l;
            o->flags |= FMD_OVLP_F_FIXED;
            st = 0;
        }
    }
}

// ------------------------------------------------------------ phase C: check_left_simple
// unitig.c:186-204 for the edge (strand -> its unique neighbour): collect, walking the neighbour
// forward from its first base, the reads that END inside it with >= min_match bases (its left
// neighbours), then pull them back over the strand's bases left of the overlap; any of them that
// neither ends nor continues with the strand's base is a backward bifurcation.  A pure function of
// the strand once its neighbour is unique, so the deterministic host walk reads it from the table:
// rec.reserved = 0 (check_left_simple returns 0), 1 (returns -1), 2 (not applicable).
enum { CL_IDLE = 0, CL_FWD, CL_PICK, CL_BWD };

__global__ __launch_bounds__(64) void k_ovl_cls(FmdIndexView ix, size_t n, int min_match, uint32_t cap, fmd_intv_t *__restrict__ listA,
                                                fmd_intv_t *__restrict__ listB, fmd_ovlp_rec_t *__restrict__ rec,
                                                const uint8_t *__restrict__ seq, uint32_t seq_stride, uint32_t *__restrict__ queue)
{
    FMD_DECLARE_WAVE_LDS();
    size_t sid = 0;
    int st = CL_IDLE, rbeg = 0, s_l = 0, depth = 0, i = 0;
    uint32_t prev_n = 0, curr_n = 0, j = 0;
    uint64_t x0 = 0, x1 = 0, sz = 0;
    fmd_intv_t *prev = nullptr, *curr = nullptr;
    const uint8_t *s = nullptr;
    bool exhausted = false;
    FmdTickets tk_;
    fmd_tickets_init(tk_, queue);
    for (;;) {
        const size_t my = fmd_tickets_take(tk_, queue, st == CL_IDLE && !exhausted);
        if (st == CL_IDLE && !exhausted) {
            if (my < n) {
                fmd_ovlp_rec_t *o = rec + my;
                if (o->reserved != 2) {}   // decided already (fmd_ovlp_link_dev): only the rows still open are looked at
                else if (o->status == 0 && o->n_nei == 1 && o->rbeg >= 0 && !(o->flags & FMD_OVLP_F_OVERFLOW) &&
                    (uint32_t)(o->len + o->ext_len) <= seq_stride) {
                    sid = my; rbeg = o->rbeg; s_l = o->len + o->ext_len;
                    s = seq + sid * (size_t)seq_stride;
                    const int c = s[rbeg];
                    x0 = ix.cnt[c]; x1 = ix.cnt[comp6(c)]; sz = ix.cnt[c + 1] - ix.cnt[c];
                    depth = 1; prev = listA + sid * (size_t)cap; curr = listB + sid * (size_t)cap; prev_n = curr_n = 0;
                    if (rbeg + 1 < s_l) st = CL_FWD;
                    else { o->reserved = 0; } // a one-base neighbour cannot collect anything
                } else o->reserved = 2;
            } else exhausted = true;
        }
        while (st == CL_PICK) {
            if (j < prev_n) { uint64_t inf; load_entry(prev + j, x0, x1, sz, inf); st = CL_BWD; }
            else { // next base to the left (unitig.c:194-202)
                fmd_intv_t *t = prev; prev = curr; curr = t;
                prev_n = curr_n; curr_n = 0; j = 0; --i;
                if (i < 0 || prev_n == 0) { rec[sid].reserved = 0; st = CL_IDLE; }
            }
        }
        if (__ballot(st != CL_IDLE) == 0) { if (__ballot(!exhausted) == 0) break; else continue; }
        uint64_t qk = NONE64, ql = NONE64;
        if (st == CL_FWD) { qk = x1 - 1; ql = x1 - 1 + sz; }
        else if (st == CL_BWD) { qk = x0 - 1; ql = x0 - 1 + sz; }
        const FmdRank2 r = fmd_wave_rank2_fetch(ix, fmd_lds, qk, ql);
        if (st == CL_IDLE) continue;
        // the symbol this step extends by: forward along the neighbour, or backward over the strand
        const int c = st == CL_FWD ? comp6(s[rbeg + depth]) : s[i];
        // Child sizes sc[], rank_c(k) and -- where a candidate may be pushed -- rank_$(k).  Narrow interval
        // (all but the first ~log4(n) forward steps): one 64-position window of the lane's block image(s)
        // and one or two single-symbol ranks instead of two six-symbol block ranks.
        uint64_t sc[6], tkc, tk0 = 0;
        if (sz <= 63) {
            const uint64_t a0 = st == CL_FWD ? x1 : x0;
            uint4 wa, wb, wc;
            grp_window(r.bk, r.t, r.bl, r.tl, r.blk_k, r.blk_l, r.hk, r.hl && r.blk_l != r.blk_k, r.blk_k, r.nk - 1, wa, wb, wc); // window at a0 = (a0 - 1) + 1
            const uint32_t sh = (uint32_t)a0 & 31;
            const uint64_t m = (1ull << (int)sz) - 1;
            const uint64_t X = win64(wa.x, wb.x, wc.x, sh), Y = win64(wa.y, wb.y, wc.y, sh), Z = win64(wa.z, wb.z, wc.z, sh);
            const uint64_t lo = ~Z & m, hi = Z & ~Y & m;
            sc[0] = __popcll(lo & ~Y & ~X); sc[1] = __popcll(lo & ~Y & X); sc[2] = __popcll(lo & Y & ~X); sc[3] = __popcll(lo & Y & X);
            sc[4] = __popcll(hi & ~X); sc[5] = __popcll(hi & X);
            tkc = fmd_block_rank1(r.bk, r.t, r.nk, c, r.blk_k);
            if (st == CL_FWD && depth >= min_match && sc[0]) tk0 = fmd_block_rank1(r.bk, r.t, r.nk, 0, r.blk_k);
        } else {
            uint64_t tk[6] = {0, 0, 0, 0, 0, 0}, tl[6] = {0, 0, 0, 0, 0, 0};
            if (r.hk) fmd_block_rank6<false>(r.bk, r.t, r.nk, tk, r.blk_k);
            if (r.hl) fmd_block_rank6<false>(r.bl, r.tl, r.nl, tl, r.blk_l);
#pragma unroll
            for (int a = 0; a < 6; ++a) sc[a] = tl[a] - tk[a];
            tkc = sel6(c, tk[0], tk[1], tk[2], tk[3], tk[4], tk[5]);
            tk0 = tk[0];
        }
        const uint64_t szc = sel6(c, sc[0], sc[1], sc[2], sc[3], sc[4], sc[5]);
        // coordinate of child c on the strand that is not extended: running sum in the order $,T,G,C,A,N (exact.c:81-86)
        uint64_t before = 0;
        if (c != 0) before += sc[0];
        if (c == 3 || c == 2 || c == 1 || c == 5) before += sc[4];
        if (c == 2 || c == 1 || c == 5) before += sc[3];
        if (c == 1 || c == 5) before += sc[2];
        if (c == 5) before += sc[1];
        const uint64_t nxc = sel6(c, ix.cnt[0], ix.cnt[1], ix.cnt[2], ix.cnt[3], ix.cnt[4], ix.cnt[5]) + tkc;
        if (st == CL_FWD) { // overlap_intv(at5 = 1, inc_sentinel = 1), unitig.c:38-64
            bool end_fwd = szc == 0;
            if (!end_fwd) {
                if (depth >= min_match && sc[0]) {
                    if (prev_n < cap) store_entry(prev + prev_n, x0, ix.cnt[0] + tk0, sc[0], 0);
                    ++prev_n;
                }
                x1 = nxc; x0 += before; sz = szc;   // ik = ok[c] (forward)
                ++depth;
                end_fwd = rbeg + depth == s_l;
            }
            if (end_fwd) {
                if (prev_n > cap) { rec[sid].flags |= FMD_OVLP_F_OVERFLOW; rec[sid].reserved = 2; st = CL_IDLE; }
                else if (prev_n == 0 || rbeg == 0) { rec[sid].reserved = 0; st = CL_IDLE; }
                else { i = rbeg - 1; j = 0; curr_n = 0; st = CL_PICK; }
            }
        } else { // CL_BWD: one collected interval against base s[i] (unitig.c:196-200)
            if (sc[0] + szc != sz) { rec[sid].reserved = 1; st = CL_IDLE; } // potential backward bifurcation
            else {
                if (curr_n < cap) store_entry(curr + curr_n, nxc, x1 + before, szc, 0);
                ++curr_n; ++j;
                st = CL_PICK;
            }
        }
    }
}

// ------------------------------------------------------------------------------- launchers
void fmd_launch_nei_slow(const NeiArgs &a, hipStream_t st, uint32_t *queue, int late)
{
    const uint32_t *list = late ? a.late : a.cl.lslow, *list_n = a.cnt(FMD_CLS_SLOW, late ? FMD_CW_LATE : FMD_CW_COUNT);
    k_ovl_nei<<<a.grid, 64, 0, st>>>(a.ix, a.np, a.min_match, a.srev, a.stride_r, a.cap, a.listA, a.listB, a.rec, a.nei, a.max_nei, a.seq, a.seq_stride, queue, list, list_n, a.gidx);
}
void fmd_launch_nei_fix(const NeiArgs &a, hipStream_t st, uint32_t *queue)
{
    k_ovl_fix<<<a.grid, 64, 0, st>>>(a.ix, a.fix, a.cnt(FMD_CLS_SLOW, FMD_CW_FIX), a.srev, a.stride_r, a.rec, a.nei, a.max_nei, a.seq, a.seq_stride, queue, a.gidx);
}
void fmd_launch_check_left(const NeiArgs &a, hipStream_t st, uint32_t *queue)
{
    k_ovl_cls<<<a.grid, 64, 0, st>>>(a.ix, a.np, a.min_match, a.cap, a.listA, a.listB, a.rec, a.seq, a.seq_stride, queue);
}
