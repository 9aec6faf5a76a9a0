// What the units that look one key up in several tables at once share (seq_cov.hip, presence.hip): the tables as a kernel argument,
// slot_of (kmer_device.h) for NT tables of one k with the home slots' reads all in flight together, and table_get's rule behind an
// occupied home slot; on the host the checks of a list of contexts, what makes their tables ready, and the kernels' dispatch.
#pragma once
#include "context.h"

template <int NT>
struct Tables {
    TableView t[NT];
};

// packed keys: the tables whose regions are minimizer bins (mm_k = k); hash keys never are, by_key_ready saw to it
template <int MODE, int NT>
__device__ __forceinline__ uint32_t bin_tables(const Tables<NT> &tv)
{
    uint32_t bins = 0;
#pragma unroll
    for (int t = 0; t < NT; t++) bins |= (MODE == KEY_PACKED && tv.t[t].mm_k != 0 ? 1u : 0u) << t;
    return bins;
}

// slot_of (kmer_device.h) for NT tables of one k: the key's hash and its minimizer bin are worked out once, and the home slots of
// all tables are loaded before any of them is looked at.  hit(t, count) is called for every table t whose home slot holds the key,
// with the count as stored.  `of` says where a table's shift and n_regions wait: of.shift(t), of.n_regions(t), t a constant (the
// kernels keep them in different places, each for its registers).
template <int MODE, int NT, class Of, class Hit>
__device__ __forceinline__ uint32_t home_slots(const Tables<NT> &tv, uint32_t bins, uint64_t key, int k, const Of &of, uint64_t (&at)[NT], Hit &&seen)
{
    const uint64_t mix = fmix64(key);
    const uint64_t bin = bins ? sk_bin(sk_hmin_of_kmer(key, k)) : 0;
    const uint64_t home = sk_home(key);
    uint4 raw[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
        at[t] = !(bins >> t & 1) ? mix >> of.shift(t) : (((bin * of.n_regions(t)) >> 32) << MC_REGION_LG) | home;
#pragma unroll
    for (int t = 0; t < NT; t++) raw[t] = *reinterpret_cast<const uint4 *>(tv.t[t].slots + at[t]);
    uint32_t behind = 0;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint64_t cur = ((uint64_t)raw[t].y << 32) | raw[t].x;
        const bool there = cur == key && (MODE == KEY_PACKED || key != EMPTY_KEY);
        seen(t, there, raw[t].z);
        if (!there && (cur != EMPTY_KEY || (MODE != KEY_PACKED && key == EMPTY_KEY))) behind |= 1u << t;  // (or the key is the free slot's mark)
    }
    return behind;
}

// What a look-up behind the home slot answers.  COUNT: what table_get answers, -1 when the key is absent, else min(32767, count)
// (seq-cov takes max(c, 0)).  Otherwise only whether the key is there, a stored count of 0 included: the count is then never
// loaded, and a bool keeps k_presence<KEY_PACKED, 3> at its 20 vector registers where 0 / -1 in an int gave 22.
template <bool COUNT>
struct Behind {
    using type = typename std::conditional<COUNT, int, bool>::type;
    static __device__ __forceinline__ type absent() { return COUNT ? (type)-1 : (type)0; }
    static __device__ __forceinline__ type found(unsigned long long count) { return COUNT ? (type)(count > 32767ull ? 32767 : (int)count) : (type)1; }
};

// table_get's probing rule (kmer_device.h) behind the home slot `s`, which the caller has found occupied by another key.  Scalars,
// not a TableView: one copy of the loops serves all the tables.  (table_get keeps its own copy of the loop: on this one, k_get and
// the k_classify kernels come out with other register counts.)
template <bool COUNT>
__device__ __forceinline__ typename Behind<COUNT>::type probe_behind_home(const Slot *__restrict__ slots, uint32_t rmask, uint32_t n_regions, uint64_t key, uint64_t s)
{
    uint64_t base = s & ~(uint64_t)rmask;
    const uint64_t home = s & rmask;
    const uint32_t max_probes = rmask + 1 < TABLE_MAX_PROBES ? rmask + 1 : TABLE_MAX_PROBES;
    for (uint32_t hop = 0; hop < TABLE_CHAIN; hop++, base = next_region_base(base, rmask, n_regions), s = base | home)
    for (uint32_t probe = 0; probe < max_probes; probe++) {
        if (hop | probe) {
            const uint4 r = *reinterpret_cast<const uint4 *>(slots + s);
            const uint64_t cur = ((uint64_t)r.y << 32) | r.x;
            if (cur == key) return Behind<COUNT>::found(r.z);
            if (cur == EMPTY_KEY) return Behind<COUNT>::absent();
        }
        s = base | ((s + 1) & rmask);
    }
    return Behind<COUNT>::absent();
}

// table_get for a table of h.behind, from the key's home slot `s` there
template <int MODE, bool COUNT>
__device__ __forceinline__ typename Behind<COUNT>::type get_behind_home(const Slot *__restrict__ slots, const unsigned long long *empty_cnt, uint32_t rmask,
                                                                        uint32_t n_regions, uint64_t key, uint64_t s)
{
    if (MODE != KEY_PACKED && key == EMPTY_KEY) {  // (table_get: such a hash is counted beside the table)
        const unsigned long long e = *empty_cnt;
        return e == 0 ? Behind<COUNT>::absent() : Behind<COUNT>::found(e);
    }
    return probe_behind_home<COUNT>(slots, rmask, n_regions, key, s);
}

// ---------------------------------------------------------------------------------------------------- host side

template <int NT>
Tables<NT> tables_view(mc_ctx *const *tables)
{
    Tables<NT> tv;
    for (int t = 0; t < NT; t++) tv.t[t] = tables[t]->view();
    return tv;
}

// f(key mode, number of tables), both as constants: for_key_mode (context.h) times 1 .. 4 tables
template <typename F>
void for_key_mode_and_tables(int key_mode, uint32_t n_tables, F &&f)
{
    for_key_mode(key_mode, [&](auto mode) {
        switch (n_tables) {
        case 1: f(mode, std::integral_constant<int, 1>()); break;
        case 2: f(mode, std::integral_constant<int, 2>()); break;
        case 3: f(mode, std::integral_constant<int, 3>()); break;
        default: f(mode, std::integral_constant<int, 4>()); break;
        }
    });
}

// null contexts and their number; the message goes to tables[0] when there is one
inline int check_tables(const char *api, uint32_t max_tables, mc_ctx *const *tables, uint32_t n_tables)
{
    if (!tables || n_tables == 0 || n_tables > max_tables) {
        mc_ctx *c0 = tables && n_tables ? tables[0] : nullptr;
        if (c0) {
            std::lock_guard<std::mutex> g(c0->mu);
            return fail(c0, MC_EINVAL, "%s: %u tables (1 .. %d)", api, n_tables, (int)max_tables);
        }
        return MC_EINVAL;
    }
    if (!tables[0]) return MC_EINVAL;
    for (uint32_t t = 1; t < n_tables; t++)
        if (!tables[t]) {
            std::lock_guard<std::mutex> g(tables[0]->mu);
            return fail(tables[0], MC_EINVAL, "%s: table %u is null", api, t);
        }
    return MC_OK;
}

// what the tables of one call must share, and that they are counted (under the caller's TablesLock, as prepare_tables)
inline int tables_agree(const char *api, mc_ctx *const *tables, uint32_t n_tables)
{
    mc_ctx *c = tables[0];
    for (uint32_t t = 1; t < n_tables; t++)
        if (tables[t]->cfg.k != c->cfg.k || tables[t]->cfg.key_mode != c->cfg.key_mode || tables[t]->cfg.device != c->cfg.device)
            return fail(c, MC_EINVAL, "%s: table %u has k = %d, key mode %d, device %d; table 0 has %d, %d, %d", api, t, tables[t]->cfg.k,
                        tables[t]->cfg.key_mode, tables[t]->cfg.device, c->cfg.k, c->cfg.key_mode, c->cfg.device);
    for (uint32_t t = 0; t < n_tables; t++)
        if (!tables[t]->finalized) return fail(c, MC_ESTATE, "%s: call mc_finalize_counts on table %u first", api, t);
    return MC_OK;
}

// every distinct table ready for look-ups by key from a kernel on table 0's stream
inline int prepare_tables(const char *api, mc_ctx *c, const TablesLock &lock)
{
    HIPCHK(c, hipSetDevice(c->cfg.device));
    for (mc_ctx *x : lock.distinct) {
        // (hash keys in minimizer bins: the table moves to hash-prefix regions, once; an empty table that was never written is filled)
        int rc = by_key_ready(x);
        if (!rc) rc = materialize(x);
        if (rc) return x == c ? rc : fail(c, rc, "%s: %s", api, x->err.c_str());
        if (x != c) HIPCHK(c, hipStreamSynchronize(x->stream));  // (its own stream did that; the kernel runs on table 0's)
    }
    return MC_OK;
}
