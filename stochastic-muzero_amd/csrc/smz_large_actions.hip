// smz_large_actions.hip -- the step-wise tree kernels for 1 <= A <= SMZ_MAX_ACTIONS_LARGE actions (smz_create_large_actions).
//
// Execution shape: ONE wavefront per tree, one wavefront per workgroup (B workgroups).  The per-lane kernels of smz_kernels.hip
// keep a tree's A-wide arrays in registers, which stops at A = 32; here the lanes split the A-wide loops and the arrays live
// in this wave's LDS.  What numpy defines as sequential stays sequential (the float64 cumsum of RandomState.choice, the
// Dirichlet gammas and their sum, the backup's value chain); every lane then computes the same scalar values, so control flow
// stays uniform over the wave.  Everything else -- normalisation, the searchsorted of a round's draws, the pUCT scores of a
// level, the one-hot network input -- runs a child or a draw per lane.  The arithmetic is smz_device.hpp's (puct_score,
// legacy_gamma, np_sum, the glibc math), called, not restated: the trees are bit-identical to the per-lane kernels'.
//
// Tree layout, node ids and hidden rows are those of smz_device.hpp.  One difference: a path record names its child as
// block << kLaSlotBits | slot (a root slot may exceed 255); smz_debug_dump_tree decodes it by the handle's kind.
//
// Random words: the wave keeps its tree's 624 MT19937 words in LDS for the launch and twists them 64 at a time in place (the
// words i .. i + 63 read words i + 397 mod 624 of the same pass only at least 227 words back, so a 64-word chunk is
// parallel-safe), then writes them back with the (ready << 16 | idx) position of the per-lane kernels.  Philox handles
// compute each word where it is needed (philox_word).  Both consume exactly the per-lane kernels' words, in their order.
//
// Build: same flags as smz_kernels.hip (-ffp-contract=off: no fused multiply-add).
#include "smz_common.hpp"
#include "smz_handle.hpp"

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
__device__ inline LaLds la_lds(int A) {
    const int ap = la_pad(A);
    char *base = reinterpret_cast<char *>(smz_dyn_lds);
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

// one wavefront per workgroup: a fence + wave barrier orders the LDS traffic between lanes
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
// root (monte_carlo_tree_search.py:179-225): root_init_tree
// ---------------------------------------------------------------------------------------------------------------
template <bool PHX>
__global__ void __launch_bounds__(kWave) k_root_init_la(Params P, const float *hidden, const float *policy,
                                                        const double *noise_override, int train) {
    const int tree = blockIdx.x, lane = la_lane();
    if (tree >= P.B || !tree_active(P, tree)) return;
    const int A = P.A;
    const LaLds L = la_lds(A);
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
    uint32_t *rb = tree_base(P, tree);
    la_normalise_policy(policy + (size_t)tree * A, A, L);
    int32_t *vi = (int32_t *)rb;
    float *fs = (float *)rb;
    for (int a = lane; a < A; a += kWave) {
        vi[2 * a] = 0;
        fs[2 * a + 1] = 0.f;
        fs[2 * A + a] = 0.f;
        fs[3 * A + a] = L.f[a];
        vi[4 * A + a] = 0;
    }
    la_choice(R, A, A, L);          // sorted result is 0..A-1; only the draws matter (mcts:208)
    double *rp = (double *)(rb + P.rp_off);
    if (!(train && P.sims > 0))
        for (int a = lane; a < A; a += kWave) rp[a] = (double)L.f[a];
    R.save(P, tree);
    if (lane == 0) {
        TreeHdr h;
        h.n_exp = 0;
        h.path_len = 0;
        h.mn = __builtin_inff();
        h.mx = -__builtin_inff();
        h.root_visit = 0;
        h.root_value_sum = 0.f;
        h.pad0 = h.pad1 = 0;
        P.hdr[tree] = h;
    }
    if (P.S > 0 && hidden) la_copy_row(hidden + (size_t)tree * P.S, P.hidden + (size_t)tree * P.N * P.hs, P.S);
}

// ... and its Dirichlet noise (mcts:216-225), a launch of its own behind it (train, num_simulations > 0): the glibc log / pow of
// the gammas beside the choice rounds would not fit the scalar registers
template <bool ONE, bool PHX>
__global__ void __launch_bounds__(kWave) k_root_noise_la(Params P, const double *noise_override) {
    const int tree = blockIdx.x, lane = la_lane();
    if (tree >= P.B || !tree_active(P, tree)) return;
    const int A = P.A;
    const LaLds L = la_lds(A);
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
    uint32_t *rb = tree_base(P, tree);
    // A legacy gammas in stream order, summed in the same order (one chain: la_cumsum's last entry)
    la_dirichlet_gammas<ONE>(R, P.alpha, A, L.d0);
    la_cumsum(L.d0, L.d1, A);
    const double inv = 1.0 / L.d1[A - 1];
    const double *ov = noise_override ? noise_override + (size_t)tree * A : nullptr;
    double *rp = (double *)(rb + P.rp_off);
    for (int a = lane; a < A; a += kWave) {
        const double n = ov ? ov[a] : L.d0[a] * inv;
        const float scaled = __uint_as_float(rb[3 * A + a]) * P.keep32;
        rp[a] = (double)scaled + n * P.frac;
    }
    R.save(P, tree);
}

// ---------------------------------------------------------------------------------------------------------------
// selection (monte_carlo_tree_search.py:228-267): select_tree, a child per lane
// ---------------------------------------------------------------------------------------------------------------
template <bool PHX>
__global__ void __launch_bounds__(kWave) k_select_la(Params P, float *parent_hidden, int32_t *last_action, uint8_t *branch,
                                                     float *mlp_input) {
    const int tree = blockIdx.x, lane = la_lane();
    if (tree >= P.B) return;
    if (!tree_active(P, tree)) {
        if (P.ids_out && lane == 0) { P.ids_out[2 * (size_t)tree] = -1; P.ids_out[2 * (size_t)tree + 1] = -1; }
        return;
    }
    const int A = P.A, K = P.K;
    const LaLds L = la_lds(A);
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
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
    R.save(P, tree);
    if (lane == 0) {
        P.hdr[tree].path_len = depth;
        if (last_action) last_action[tree] = action;
        if (branch) branch[tree] = (uint8_t)depth_flag(depth - 1);
        if (P.ids_out) { P.ids_out[2 * (size_t)tree] = leaf_id; P.ids_out[2 * (size_t)tree + 1] = parent_id; }
    }
    if (P.S > 0 && (parent_hidden || mlp_input)) {
        const int S = P.S, W = S + A;
        const float *src = P.hidden + ((size_t)tree * P.N + parent_id) * P.hs;
        for (int i = lane; i < (mlp_input ? W : S); i += kWave) {
            const float v = i < S ? src[i] : ((i - S) == action ? 1.0f : 0.0f);
            if (mlp_input) mlp_input[(size_t)tree * W + i] = v;
            if (parent_hidden && i < S) parent_hidden[(size_t)tree * S + i] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// expansion + backup (monte_carlo_tree_search.py:282-308): expand_backup_tree; MP = the multi-player sign rule
// ---------------------------------------------------------------------------------------------------------------
template <bool MP, bool PHX>
__global__ void __launch_bounds__(kWave) k_expand_backup_la(Params P, const float *hidden, const float *reward,
                                                            const float *policy, const float *value) {
    const int tree = blockIdx.x, lane = la_lane();
    if (tree >= P.B || !tree_active(P, tree)) return;
    const int A = P.A, K = P.K;
    const LaLds L = la_lds(A);
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
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
    const float leaf_reward = pflag ? (reward ? reward[tree] : 0.0f) : 0.0f;   // the afterstate branch never assigns one
    const int leaf = la_node_id(P, leaf_loc);
    if (lane == 0) {
        const int lb = (int)(leaf_loc >> kLaSlotBits), ls = (int)(leaf_loc & ((1u << kLaSlotBits) - 1u));
        const int lc = (lb == 0) ? A : K;
        uint32_t *lp = block_ptr(P, tb, lb);
        lp[4 * lc + ls] = (uint32_t)(e + 1);
        lp[2 * lc + ls] = __float_as_uint(leaf_reward);
        // ---- backup, leaf -> root: the float32 value chain is sequential ----
        float v = value[tree];
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
    la_normalise_policy(policy + (size_t)tree * A, A, L);
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
    R.save(P, tree);
    if (P.S > 0 && hidden) la_copy_row(hidden + (size_t)tree * P.S, P.hidden + ((size_t)tree * P.N + leaf) * P.hs, P.S);
}

// ---------------------------------------------------------------------------------------------------------------
// post-search policy / action (game.py:179-232): act_tree
// ---------------------------------------------------------------------------------------------------------------
template <bool PHX>
__global__ void __launch_bounds__(kWave) k_act_la(Params P, double temperature, int32_t *action_out, double *policy_out,
                                                  double *child_visits_out, float *root_value_out) {
    const int tree = blockIdx.x, lane = la_lane();
    if (tree >= P.B || !tree_active(P, tree)) return;
    const int A = P.A;
    const LaLds L = la_lds(A);
    const uint32_t *rb = tree_base(P, tree);
    const double *rp = (const double *)(rb + P.rp_off);
    double *vis = L.d0, *pol = L.d1, *cdf = L.d2;
    for (int a = lane; a < A; a += kWave) vis[a] = (double)(int32_t)rb[2 * a];
    la_sync();
    const double vsum = la_sum<double>(vis, A);
    const bool from_visits = !(vsum <= 1.0);
    bool eq = true;
    const bool table = temperature >= 0.3 && from_visits && P.pow_table;
    for (int a = lane; a < A; a += kWave) pol[a] = table ? P.pow_table[(int32_t)rb[2 * a]] : (from_visits ? vis[a] : rp[a]);
    if (temperature >= 0.3 && !table) {                 // (numpy's ** = libm's pow)
        const double e = 1.0 / temperature;
        for (int a = lane; a < A; a += kWave) pol[a] = smz_glibc_pow(pol[a], e);
    }
    la_sync();
    const double ps = la_sum<double>(pol, A);
    la_sync();
    for (int a = lane; a < A; a += kWave) pol[a] = pol[a] / ps;
    la_sync();
    for (int a = lane; a < A; a += kWave) eq = eq && (pol[a] == pol[0]);
    const bool all_equal = __ballot(!eq) == 0ull;
    LaRng<PHX> R;
    R.load(P, tree, L.mt);
    int pick = 0;
    if (temperature > 0.1 || all_equal) {
        pick = la_sample_cdf(pol, cdf, A, R.random_sample());
    } else {
        double best = 0.0;
        int bj = -1;
        for (int a = lane; a < A; a += kWave) if (bj < 0 || pol[a] > best) { best = pol[a]; bj = a; }
        la_argmax_first(best, bj);
        pick = bj;
    }
    R.save(P, tree);
    if (action_out && lane == 0) action_out[tree] = pick;
    if (policy_out) for (int a = lane; a < A; a += kWave) policy_out[(size_t)tree * A + a] = pol[a];
    if (child_visits_out) {
        if (vsum >= 3.0) {
            for (int a = lane; a < A; a += kWave) child_visits_out[(size_t)tree * A + a] = vis[a] / vsum;
        } else {
            for (int a = lane; a < A; a += kWave) cdf[a] = rp[a];
            la_sync();
            const double s = la_sum<double>(cdf, A);
            for (int a = lane; a < A; a += kWave) child_visits_out[(size_t)tree * A + a] = rp[a] / s;
        }
    }
    if (root_value_out && lane == 0) {
        const TreeHdr h = P.hdr[tree];
        root_value_out[tree] = h.root_visit ? h.root_value_sum / (float)h.root_visit : 0.0f;
    }
}

inline dim3 la_grid(const Params &P) { return dim3((unsigned)P.B); }

}  // namespace

// ---- entry points of smz_kernels.hip for large-action handles (smz_handle::large_actions) --------------------------------
#define SMZ_LA_LAUNCH(KERNEL, P, ...)                                                                                         \
    do {                                                                                                                     \
        if ((P).philox) hipLaunchKernelGGL((KERNEL<__VA_ARGS__ true>), la_grid(P), dim3(kWave), la_lds_bytes((P).A), (hipStream_t)stream, \
                                          (P), SMZ_LA_ARGS);                                                                  \
        else hipLaunchKernelGGL((KERNEL<__VA_ARGS__ false>), la_grid(P), dim3(kWave), la_lds_bytes((P).A), (hipStream_t)stream, \
                                (P), SMZ_LA_ARGS);                                                                            \
    } while (0)

int smz_internal_la_root_init(smz_handle *h, const float *hidden_dev, const float *policy_dev, const double *noise_override_dev,
                              int train, smz_stream stream) {
#define SMZ_LA_ARGS hidden_dev, policy_dev, noise_override_dev, train
    SMZ_LA_LAUNCH(k_root_init_la, h->P, );
#undef SMZ_LA_ARGS
    if (train && h->P.sims > 0) {
#define SMZ_LA_ARGS noise_override_dev
        if (h->P.alpha == 1.0) SMZ_LA_LAUNCH(k_root_noise_la, h->P, true,);      // Dirichlet(1): one uniform per gamma
        else SMZ_LA_LAUNCH(k_root_noise_la, h->P, false,);
#undef SMZ_LA_ARGS
    }
    return launch_check();
}

int smz_internal_la_select(smz_handle *h, float *parent_hidden_dev, int32_t *last_action_dev, uint8_t *branch_dev,
                           float *mlp_input_dev, smz_stream stream) {
#define SMZ_LA_ARGS parent_hidden_dev, last_action_dev, branch_dev, mlp_input_dev
    SMZ_LA_LAUNCH(k_select_la, h->P, );
#undef SMZ_LA_ARGS
    return launch_check();
}

int smz_internal_la_expand_backup(smz_handle *h, const float *hidden_dev, const float *reward_dev, const float *policy_dev,
                                  const float *value_dev, smz_stream stream) {
#define SMZ_LA_ARGS hidden_dev, reward_dev, policy_dev, value_dev
    if (h->P.n_cycle > 1) SMZ_LA_LAUNCH(k_expand_backup_la, h->P, true,);     // multi-player backup (smz_set_players)
    else SMZ_LA_LAUNCH(k_expand_backup_la, h->P, false,);
#undef SMZ_LA_ARGS
    return launch_check();
}

int smz_internal_la_act(smz_handle *h, const Params &P, double temperature, int32_t *action_dev, double *policy_dev,
                        double *child_visits_dev, float *root_value_dev, smz_stream stream) {
#define SMZ_LA_ARGS temperature, action_dev, policy_dev, child_visits_dev, root_value_dev
    SMZ_LA_LAUNCH(k_act_la, P, );
#undef SMZ_LA_ARGS
    return launch_check();
}
#undef SMZ_LA_LAUNCH
