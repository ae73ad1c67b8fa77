// smz_large_actions_device.hpp -- device code of the wave-per-tree tree kernels for up to SMZ_MAX_ACTIONS_LARGE actions, shared by
// the step-wise kernels (k_select_la, k_expand_backup_la, ...: smz_large_actions.hip, whose header comment describes the
// execution shape and the random stream) and the whole-search kernel (k_search_mlp_large, smz_mlp_large_search.hip).  A tree is
// one wavefront's work with all its A-wide state in that wavefront's LDS (LaLds, any byte offset of the dynamic LDS); the
// selection and the expansion + backup of a round are device functions here (la_select_tree, la_expand_backup_tree) that take
// the tree, its LaLds and a LIVE LaRng: the step-wise kernels load the generator, call one of them and save; the whole-search
// kernel loads once, calls them round after round and saves once.  Both compile them with the same flags
// (-ffp-contract=off), so a tree goes through the same arithmetic on either path.
#pragma once
#include "smz_common.hpp"

namespace {

constexpr int kLaSlotBits = 10;                      // path records: block << 10 | slot
constexpr int kLaMtWords = 640;                      // LDS words of the MT state (624, padded to 16 bytes)
constexpr int kLaWindow = 128;                       // most words one prepare() makes readable
static_assert(kLaWindow + kWave - 1 <= kMtN - kMtM, "twist-ahead window beyond what smz_get_rng_state can undo");

static_assert(SMZ_MAX_ACTIONS_LARGE <= (1 << kLaSlotBits), "a slot must fit the path record's slot field");

// per-wave LDS: [mt 640 u32] [d0 f64 Ap] [d1 f64 Ap] [d2 f64 Ap] [f f32 Ap] [i i32 Ap] [u8 Ap]   (Ap = A rounded up to 64)
struct LaLds {
    uint32_t *mt;
    double *d0, *d1, *d2;
    float *f;
    int32_t *i;
    uint8_t *u;
};
__host__ __device__ inline int la_pad(int n) { return (n + 63) & ~63; }
__host__ __device__ inline size_t la_lds_bytes(int A) {
    const size_t ap = (size_t)la_pad(A);
    return (size_t)kLaMtWords * 4 + ap * (3 * 8 + 4 + 4 + 1);
}
// (byte_off: where this wavefront's area starts in the dynamic LDS, a multiple of 16)
__device__ inline LaLds la_lds(int A, size_t byte_off = 0) {
    const int ap = la_pad(A);
    char *base = reinterpret_cast<char *>(smz_dyn_lds) + byte_off;
    LaLds L;
    L.mt = reinterpret_cast<uint32_t *>(base);
    L.d0 = reinterpret_cast<double *>(base + kLaMtWords * 4);
    L.d1 = L.d0 + ap;
    L.d2 = L.d1 + ap;
    L.f = reinterpret_cast<float *>(L.d2 + ap);
    L.i = reinterpret_cast<int32_t *>(L.f + ap);
    L.u = reinterpret_cast<uint8_t *>(L.i + ap);
    return L;
}

// a tree is one wavefront's: a fence + wave barrier orders its LDS traffic between the lanes (and, in a workgroup of several
// wavefronts, completes the wavefront's global stores: what lane 0 stored to the tree, every lane may then load)
__device__ __forceinline__ void la_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int la_lane() { return (int)(threadIdx.x & (kWave - 1)); }

// ---------------------------------------------------------------------------------------------------------------
// The tree's random stream, drawn by the whole wave.  Every lane holds the same (uniform) position.
// prepare(n) makes words used .. used + n - 1 readable (n <= kLaWindow), word(o) is word used + o, advance(n) consumes n.
// A launch thus leaves at most kLaWindow + 63 words twisted ahead: smz_get_rng_state takes a window of up to 227.
// PHX: the handle draws from Philox (a template argument: the generator's state stays out of the other kernels' registers).
// ---------------------------------------------------------------------------------------------------------------
template <bool PHX>
struct LaRng {
    static constexpr bool philox = PHX;
    uint32_t *mt;          // LDS (MT19937)
    int idx0, used, ahead; // position at launch; words drawn since; words from idx0 on already twisted
    uint32_t block0, k0, k1;

    __device__ void load(const Params &P, int tree, uint32_t *lds_mt) {
        const int packed = P.rng_pos[tree];
        idx0 = packed & 0xffff;
        ahead = packed >> 16;
        used = 0;
        mt = lds_mt;
        block0 = k0 = k1 = 0u;
        if constexpr (PHX) {
            block0 = P.rng_block[tree];
            k0 = P.rng_key[2 * tree];
            k1 = P.rng_key[2 * tree + 1];
        } else {
            const uint32_t *g = P.mt + (size_t)tree * kMtN;
            for (int i = la_lane(); i < kMtN; i += kWave) mt[i] = g[i];
            la_sync();
        }
    }
    __device__ void save(const Params &P, int tree) const {
        const int pos = idx0 + used;
        if constexpr (PHX) {
            if (la_lane() == 0) {
                P.rng_pos[tree] = pos % kMtN;
                P.rng_block[tree] = block0 + (uint32_t)(pos / kMtN);
            }
            return;
        }
        la_sync();
        uint32_t *g = P.mt + (size_t)tree * kMtN;
        for (int i = la_lane(); i < kMtN; i += kWave) g[i] = mt[i];
        const int ready = ahead > used ? ahead - used : 0;
        if (la_lane() == 0) P.rng_pos[tree] = (ready << 16) | (pos % kMtN);
    }
    // MT19937: twist 64 words at a time in place (all lanes read their three source words before any lane stores)
    __device__ void prepare(int n) {
        if constexpr (PHX) return;
        while (ahead < used + n) {
            const int off = ahead + la_lane();
            const int p = (idx0 + off) % kMtN;
            const int p1 = (p + 1 == kMtN) ? 0 : p + 1;
            int pm = p + kMtM;
            if (pm >= kMtN) pm -= kMtN;
            const uint32_t a = mt[p], b = mt[p1], c = mt[pm];
            la_sync();
            mt[p] = mt_twist(a, b, c);
            la_sync();
            ahead += kWave;
        }
    }
    __device__ uint32_t word(int o) const {
        const int pos = idx0 + used + o;
        if constexpr (PHX) return philox_word_compact(block0 + (uint32_t)(pos / kMtN), pos % kMtN, k0, k1);
        return mt_temper(mt[pos % kMtN]);
    }
    __device__ void advance(int n) { used += n; }
    // RandomState.random_sample(), called by every lane alike (lanes 0 and 1 fetch a word each)
    __device__ double random_sample() {
        prepare(2);
        const uint32_t w = word(la_lane() & 1);
        const double u = Rng::to_double(__builtin_amdgcn_readlane(w, 0), __builtin_amdgcn_readlane(w, 1));
        advance(2);
        return u;
    }
};

// ndarray.sum() of an LDS vector, every lane alike (numpy's pairwise order: np_sum_pairwise)
template <typename T>
__device__ inline T la_sum(const T *a, int n) { return np_sum_pairwise<T>(a, n); }

// cumsum of a float64 LDS vector: numpy's add.accumulate is ONE sequential chain, so one lane runs it
__device__ inline void la_cumsum(const double *p, double *cdf, int n) {
    la_sync();
    if (la_lane() == 0) {
        double acc = 0.0;
        for (int i = 0; i < n; i++) { acc += p[i]; cdf[i] = acc; }
    }
    la_sync();
}

// entries of cdf[0 .. n-2] <= u (sample_cdf's count; the last entry cdf[n-1] / last is 1.0 or NaN and never counts), every lane
// gets it: a binary search while the cdf is monotone (a cumsum of non-negative terms divided by a positive, finite total),
// the plain count otherwise
__device__ inline int la_count_le(const double *cdf_norm, int n, double u, bool mono) {
    if (mono) {
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf_norm[mid] <= u) lo = mid + 1; else hi = mid;
        }
        return lo;
    }
    int k = 0;
    for (int i = 0; i < n - 1; i++) k += (cdf_norm[i] <= u) ? 1 : 0;
    return k;
}
__device__ inline bool la_monotone(double last) { return last > 0.0 && last < __builtin_inf(); }

// p = (policy + 1e-12) / sum (normalise_policy): f32 into L.f, its float64 copy into L.d0
__device__ inline void la_normalise_policy(const float *policy_row, int A, const LaLds &L) {
    for (int a = la_lane(); a < A; a += kWave) L.f[a] = policy_row[a] + 1e-12f;
    la_sync();
    const float s = la_sum<float>(L.f, A);
    la_sync();
    for (int a = la_lane(); a < A; a += kWave) {
        const float v = L.f[a] / s;
        L.f[a] = v;
        L.d0[a] = (double)v;
    }
    la_sync();
}

// RandomState.choice(n, size, p=p, replace=False) (choice_noreplace's rounds): p = L.d0 (clobbered), cdf = L.d1, the
// first draw of each entry in a round = L.i, picked entries flagged in L.u.  Returns with the picks in increasing order in
// L.i[0 .. size) (np.sort of the result).
template <class RNG>
__device__ inline void la_choice(RNG &R, int n, int size, const LaLds &L) {
    const int lane = la_lane();
    for (int a = lane; a < n; a += kWave) L.u[a] = 0;
    int n_uniq = 0;
    while (n_uniq < size) {
        const int m = size - n_uniq;
        la_cumsum(L.d0, L.d1, n);
        const double last = L.d1[n - 1];
        for (int i = lane; i < n; i += kWave) {
            if (i < n - 1) L.d1[i] = L.d1[i] / last;
            L.i[i] = 0x7fffffff;
        }
        la_sync();
        const bool mono = la_monotone(last);
        for (int d0 = 0; d0 < m; d0 += kWave) {           // 64 draws per pass, in stream order
            const int nd = m - d0 < kWave ? m - d0 : kWave;
            R.prepare(2 * nd);
            int cand = 0;
            if (lane < nd) {
                const double x = Rng::to_double(R.word(2 * lane), R.word(2 * lane + 1));
                cand = la_count_le(L.d1, n, x, mono);
                atomicMin(&L.i[cand], d0 + lane);
            }
            R.advance(2 * nd);
            la_sync();
            // a draw is new iff it is the round's first draw of its entry (np.unique's first occurrence); picks zero their p
            // for the next round (the cdf of this one is already built)
            const bool keep = lane < nd && L.i[cand] == d0 + lane;
            if (keep) { L.u[cand] = 1; L.d0[cand] = 0.0; }
            n_uniq += __popcll(__ballot(keep));
            la_sync();
        }
    }
    // sorted picks: compaction of the flags in index order
    int base = 0;
    for (int a0 = 0; a0 < n; a0 += kWave) {
        const int a = a0 + lane;
        const bool f = a < n && L.u[a] != 0;
        const unsigned long long bal = __ballot(f);
        la_sync();
        if (f) L.i[base + __popcll(bal & ((1ull << lane) - 1ull))] = a;
        base += __popcll(bal);
    }
    la_sync();
}

// legacy_gamma(shape) A times in stream order into g[0 .. A): a round (four words) per lane, 32 consecutive rounds per pass; the
// gammas are the accepting rounds in order (legacy_gamma_round).  shape == 1: one uniform each, shape == 0: no words.
// ONE: shape == 1 (a compile-time switch: one pass body per instantiation)
template <bool ONE, class RNG>
__device__ inline void la_dirichlet_gammas(RNG &R, double shape, int A, double *g) {
    const int lane = la_lane();
    if (shape == 0.0) {
        for (int a = lane; a < A; a += kWave) g[a] = 0.0;
        la_sync();
        return;
    }
    constexpr bool one = ONE;
    constexpr int per = ONE ? 2 : 4;      // words per round
    constexpr int nr = kLaWindow / per;   // rounds per pass: the words of a pass stay within prepare's window
    int got = 0;
    while (got < A) {
        R.prepare(per * nr);
        const int r = lane < nr ? lane : 0;  // (lanes beyond the pass repeat round 0 and drop it)
        double x = 0.0;
        bool ok;
        const double U = Rng::to_double(R.word(per * r), R.word(per * r + 1));
        if constexpr (one) {
            x = -smz_glibc_log(1.0 - U);
            ok = true;
        } else {
            ok = legacy_gamma_round(U, Rng::to_double(R.word(per * r + 2), R.word(per * r + 3)), shape, x);
        }
        ok = ok && lane < nr;
        const unsigned long long bal = __ballot(ok);
        const int rank = __popcll(bal & ((1ull << lane) - 1ull)), n_ok = __popcll(bal);
        if (ok && got + rank < A) g[got + rank] = x;
        if (got + n_ok >= A) {            // the gamma A - 1 ends this pass: the words up to its round are consumed
            const int t = __ffsll((long long)__ballot(ok && got + rank == A - 1)) - 1;
            R.advance(per * (t + 1));
            got = A;
        } else {
            R.advance(per * nr);
            got += n_ok;
        }
    }
    la_sync();
}

// wave argmax of (score, index): the larger score, an exact tie to the larger index -- Python's max over the reference's
// (score, action, child) tuples, i.e. pick_decision's `score >= best` in child order
__device__ inline void la_argmax_last(double &best, int &pick) {
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int op = __shfl_xor(pick, off);
        if (op >= 0 && (pick < 0 || ob > best || (ob == best && op > pick))) { best = ob; pick = op; }
    }
}
// ... and np.argmax: the larger value, a tie to the SMALLER index
__device__ inline void la_argmax_first(double &best, int &pick) {
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int op = __shfl_xor(pick, off);
        if (op >= 0 && (pick < 0 || ob > best || (ob == best && op < pick))) { best = ob; pick = op; }
    }
}

// sample_cdf over an LDS vector: cumsum (one lane), then the count of cdf[i] / last <= u over i < n - 1 (a lane per entry)
__device__ inline int la_sample_cdf(const double *p, double *cdf, int n, double u) {
    la_cumsum(p, cdf, n);
    const double last = cdf[n - 1];
    int k = 0;
    for (int i = la_lane(); i < n - 1; i += kWave) k += ((cdf[i] / last) <= u) ? 1 : 0;
    for (int off = kWave / 2; off > 0; off >>= 1) k += __shfl_xor(k, off);
    return k;
}

__device__ inline int la_node_id(const Params &P, uint32_t loc) {
    const int blk = (int)(loc >> kLaSlotBits), slot = (int)(loc & ((1u << kLaSlotBits) - 1u));
    return blk == 0 ? 1 + slot : 1 + P.A + (blk - 1) * P.K + slot;
}

// one hidden row (S floats) moved by the wave
__device__ inline void la_copy_row(const float *src, float *dst, int S) {
    for (int i = la_lane(); i < S; i += kWave) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------------------------
// selection (monte_carlo_tree_search.py:228-267): select_tree, a child per lane.  Writes the path records and the header's
// path_len; returns the leaf (every lane alike).
// ---------------------------------------------------------------------------------------------------------------
struct LaLeaf {
    int parent_id, leaf_id, action, branch;      // node ids (la_node_id), the action into the leaf, 1 = dynamics / 0 = afterstate
};
template <class RNG>
__device__ inline LaLeaf la_select_tree(const Params &P, int tree, const LaLds &L, RNG &R) {
    const int lane = la_lane();
    const int A = P.A, K = P.K;
    uint32_t *tb = tree_base(P, tree);
    const float mn = P.hdr[tree].mn, mx = P.hdr[tree].mx;
    const bool norm = mx > mn;
    const float span = mx - mn;
    const PathCol rec = path_col(P, tree);
    int depth = 0, cur_visit = P.hdr[tree].root_visit, action = 0, leaf_id = 0, parent_id = 0, blk = 0;
    for (;;) {
        const bool root = blk == 0;
        const int cnt = root ? A : K;
        const uint32_t *bp = root ? tb : tb + P.rb_words + (size_t)(blk - 1) * P.eb_words;
        int pick;
        if (depth_flag(depth)) {
            // chance-flagged node: pick_chance over the block's float32 priors
            for (int j = lane; j < cnt; j += kWave) { const float om = 1.0f - __uint_as_float(bp[3 * cnt + j]); L.f[j] = om + 1e-12f; }
            la_sync();
            const float s = la_sum<float>(L.f, cnt);
            const float r = fabsf((float)((double)s / (double)cnt));
            la_sync();
            for (int j = lane; j < cnt; j += kWave) L.f[j] = __uint_as_float(bp[3 * cnt + j]) + r;
            la_sync();
            const float qs = la_sum<float>(L.f, cnt);
            for (int j = lane; j < cnt; j += kWave) L.d0[j] = (double)(L.f[j] / qs);
            la_sync();
            pick = la_sample_cdf(L.d0, L.d1, cnt, R.random_sample());
        } else {
            // decision-flagged node: pUCT over all children, one uniform per child in child order
            const double sp = P.pbc_sqrt[cur_visit];
            const double *rp = reinterpret_cast<const double *>(tb + P.rp_off);
            double best = 0.0;
            int bj = -1;
            for (int c0 = 0; c0 < cnt; c0 += kWave) {
                const int nc = cnt - c0 < kWave ? cnt - c0 : kWave;
                R.prepare(2 * nc);
                if (lane < nc) {
                    const int j = c0 + lane;
                    Kids<1> k;
                    k.vis[0] = (int32_t)bp[2 * j];
                    k.vsum[0] = __uint_as_float(bp[2 * j + 1]);
                    k.rew[0] = __uint_as_float(bp[2 * cnt + j]);
                    k.pri[0] = __uint_as_float(bp[3 * cnt + j]);
                    k.pri64[0] = root ? rp[j] : (double)k.pri[0];
                    const double u = Rng::to_double(R.word(2 * lane), R.word(2 * lane + 1));
                    const double score = puct_score<1>(k, 0, sp, norm, mn, span, P.disc32, u, nullptr);
                    if (bj < 0 || score >= best) { best = score; bj = j; }
                }
                R.advance(2 * nc);
            }
            la_argmax_last(best, bj);
            pick = bj;
        }
        const uint2 vv = *reinterpret_cast<const uint2 *>(bp + 2 * pick);
        const float pr = __uint_as_float(bp[2 * cnt + pick]);
        const int c = (int)bp[4 * cnt + pick];
        cur_visit = (int)vv.x;
        action = root ? pick : (int)bp[5 * cnt + pick];
        if (lane == 0) rec[depth] = make_uint4(((uint32_t)blk << kLaSlotBits) | (uint32_t)pick, vv.x, vv.y, __float_as_uint(pr));
        parent_id = leaf_id;
        leaf_id = root ? 1 + pick : 1 + A + (blk - 1) * K + pick;
        depth++;
        if (c == 0) break;
        blk = c;
    }
    if (lane == 0) P.hdr[tree].path_len = depth;
    return LaLeaf{parent_id, leaf_id, action, depth_flag(depth - 1)};
}

// ---------------------------------------------------------------------------------------------------------------
// expansion + backup (monte_carlo_tree_search.py:282-308): expand_backup_tree of the leaf the last la_select_tree recorded;
// MP = the multi-player sign rule.  reward / value: the networks' scalars for the leaf (the afterstate branch assigns no
// reward: ignored there); policy_row: its A policy entries.  Returns the leaf's node id (where its hidden row belongs).
// ---------------------------------------------------------------------------------------------------------------
template <bool MP, class RNG>
__device__ inline int la_expand_backup_tree(const Params &P, int tree, const LaLds &L, RNG &R, float reward, const float *policy_row,
                                            float value) {
    const int lane = la_lane();
    const int A = P.A, K = P.K;
    uint32_t *tb = tree_base(P, tree);
    TreeHdr h = P.hdr[tree];
    const PathCol rec = path_col(P, tree);
    const int len = h.path_len;
    const uint32_t leaf_loc = rec[len - 1].x;
    const int pflag = depth_flag(len - 1);
    // (the backup first: it draws no words and touches no word the expansion writes -- its multi-player state is then dead
    // before the choice rounds)
    const int e = h.n_exp;
    h.n_exp = e + 1;
    const float leaf_reward = pflag ? reward : 0.0f;   // the afterstate branch never assigns one
    const int leaf = la_node_id(P, leaf_loc);
    if (lane == 0) {
        const int lb = (int)(leaf_loc >> kLaSlotBits), ls = (int)(leaf_loc & ((1u << kLaSlotBits) - 1u));
        const int lc = (lb == 0) ? A : K;
        uint32_t *lp = block_ptr(P, tb, lb);
        lp[4 * lc + ls] = (uint32_t)(e + 1);
        lp[2 * lc + ls] = __float_as_uint(leaf_reward);
        // ---- backup, leaf -> root: the float32 value chain is sequential ----
        float v = value;
        float mn = h.mn, mx = h.mx;
        uint32_t neg = 0u;
        int pj = 0;
        if constexpr (MP) {        // as expand_backup_tree<MP>: turn of depth d = 2 (d >> 2) + ((d & 3) != 0) after the root
            const int Lc = P.n_cycle;
            int r = P.root_player ? P.root_player[tree] % Lc : 0;
            if (r < 0) r += Lc;
            neg = P.player_neg[r];
            pj = (2 * (len >> 2) + ((len & 3) != 0)) % Lc;
        }
        for (int i = len - 1; i >= 0; i--) {
            const uint4 e4 = rec[i];
            const int b = (int)(e4.x >> kLaSlotBits), sl = (int)(e4.x & ((1u << kLaSlotBits) - 1u));
            uint32_t *np = block_ptr(P, tb, b) + 2 * sl;
            const float r = (i == len - 1) ? leaf_reward : __uint_as_float(e4.w);
            float sv = v;
            if constexpr (MP) {
                if ((neg >> pj) & 1u) sv = -v;
                pj -= ((i + 1) & 3) <= 1;
                if (pj < 0) pj += P.n_cycle;
            }
            const float nvs = __uint_as_float(e4.z) + sv;
            const int nvc = (int)e4.y + 1;
            *reinterpret_cast<uint2 *>(np) = make_uint2((uint32_t)nvc, __float_as_uint(nvs));
            const float qv = nvs / (float)nvc;
            if (qv > mx) mx = qv;
            if (qv < mn) mn = qv;
            const float dv = P.disc32 * v;
            v = r + dv;
        }
        {   // the root itself (reward 0)
            const float nvs = h.root_value_sum + v;
            const int nvc = h.root_visit + 1;
            h.root_value_sum = nvs;
            h.root_visit = nvc;
            const float qv = nvs / (float)nvc;
            if (qv > mx) mx = qv;
            if (qv < mn) mn = qv;
        }
        h.mn = mn;
        h.mx = mx;
        P.hdr[tree] = h;
    }
    // ---- expansion: choice(A, K, p, replace=False), sorted ----
    la_normalise_policy(policy_row, A, L);
    la_choice(R, A, K, L);
    uint32_t *nb = tb + P.rb_words + (size_t)e * P.eb_words;
    for (int j = lane; j < K; j += kWave) {
        const int a = L.i[j];
        nb[2 * j] = 0u;
        nb[2 * j + 1] = __float_as_uint(0.f);
        nb[2 * K + j] = __float_as_uint(0.f);
        nb[3 * K + j] = __float_as_uint(L.f[a]);       // prior = un-renormalised p[a]
        nb[4 * K + j] = 0u;
        nb[5 * K + j] = (uint32_t)a;
    }
    return leaf;
}

}  // namespace
