/* Stand-alone driver of oracle/smz_oracle.c at the widths its stack arrays were enlarged for (ORC_MAX_A = 1024), meant to be
 * built with -fsanitize=address,undefined (tests/test_oracle_wide_sanitized.py): root init with Dirichlet noise, six rounds of
 * select / expand_backup and orc_act at T = 0, 0.5 and 1, at (A, K) = (1024, 1024) and (1000, 5), on both word sources.  An
 * index past an A-wide stack array, a node past the tree's capacity or a path record past sims + 2 stops the run; the
 * invariants below catch a run that stays in bounds but loses a visit or a node.  Prints one "ok:" line. */
#include <stdio.h>

#include "smz_oracle.c"

#define SIMS 6
#define S 4

static uint32_t lcg_state = 12345u;
static float lcg01(void) {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (float)(lcg_state >> 8) / 16777216.0f;
}

/* a softmax-like policy with a few dominant entries, so that `choice` without replacement needs several rounds */
static void fill_policy(float *p, int A) {
    float s = 0.f;
    for (int a = 0; a < A; a++) { float u = lcg01(); p[a] = u * u * u * u + 1e-4f; s += p[a]; }
    for (int a = 0; a < A; a++) p[a] /= s;
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "A=%d K=%d: %s failed (line %d)\n", A, K, #c, __LINE__); return 1; } } while (0)

static int run(int A, int K, int philox, long *nodes_out) {
    static float pol[ORC_MAX_A], hid[S];
    static double noise[ORC_MAX_A], policy[ORC_MAX_A], cv[ORC_MAX_A], priors[ORC_MAX_A];
    static int32_t visits[ORC_MAX_A];
    orc_cfg cfg = {A, K, S, SIMS, 19652, 1.25, 0.97, 0.3, 0.25};
    orc_tree *t = orc_tree_new(&cfg, NULL);
    CHECK(t != NULL);
    if (philox) orc_tree_seed_philox(t, 0x9E3779B97F4A7C15ull + (uint64_t)A); else orc_tree_seed(t, 77u + (uint32_t)A);
    for (int search = 0; search < 2; search++) {          /* the second search continues the stream on a reset tree */
        fill_policy(pol, A);
        for (int i = 0; i < S; i++) hid[i] = lcg01();
        orc_root_init(t, hid, pol, 1, noise);
        double ns = 0.0;
        for (int a = 0; a < A; a++) { CHECK(noise[a] >= 0.0); ns += noise[a]; }
        CHECK(fabs(ns - 1.0) < 1e-9);
        for (int s = 0; s < SIMS; s++) {
            int32_t leaf, parent, act, flag;
            float ph[S];
            orc_select(t, &leaf, &parent, &act, &flag, ph);
            CHECK(leaf > 0 && leaf < t->n_nodes && parent >= 0 && parent < leaf && act >= 0 && act < A);
            CHECK(t->path_len >= 2 && t->path_len <= SIMS + 2 && t->child_base[leaf] == 0);
            fill_policy(pol, A);
            for (int i = 0; i < S; i++) hid[i] = lcg01();
            orc_expand_backup(t, hid, lcg01() - 0.5f, pol, lcg01() - 0.5f);
            CHECK(t->n_nodes == 1 + A + (s + 1) * K && t->n_nodes <= t->N);
            const int cb = t->child_base[leaf];
            for (int j = 0; j < K; j++) {
                CHECK(t->action[cb + j] >= 0 && t->action[cb + j] < A);
                CHECK(j == 0 || t->action[cb + j] > t->action[cb + j - 1]);      /* K distinct actions, sorted */
            }
        }
        float rv;
        orc_root_stats(t, visits, priors, &rv, NULL);
        long vs = 0;
        for (int a = 0; a < A; a++) vs += visits[a];
        CHECK(vs == SIMS && t->visit[0] == SIMS);
        const double temps[3] = {0.0, 0.5, 1.0};
        for (int k = 0; k < 3; k++) {
            int32_t action;
            orc_act(t, temps[k], NULL, &action, policy, cv, &rv);
            CHECK(action >= 0 && action < A && visits[action] > 0);
            double ps = 0.0, cs = 0.0;
            for (int a = 0; a < A; a++) { ps += policy[a]; cs += cv[a]; }
            CHECK(fabs(ps - 1.0) < 1e-9 && fabs(cs - 1.0) < 1e-9);
        }
    }
    *nodes_out += t->n_nodes;
    orc_tree_free(t);
    return 0;
}

int main(void) {
    long nodes = 0;
    const int shapes[2][2] = {{1024, 1024}, {1000, 5}};
    for (int i = 0; i < 2; i++)
        for (int philox = 0; philox < 2; philox++)
            if (run(shapes[i][0], shapes[i][1], philox, &nodes)) return 1;
    orc_cfg bad = {ORC_MAX_A + 1, 2, S, SIMS, 19652, 1.25, 0.97, 0.3, 0.25};
    if (orc_tree_new(&bad, NULL) != NULL) { fprintf(stderr, "A = %d was not refused\n", bad.A); return 1; }
    printf("ok: 4 trees x 2 searches x %d rounds at (A, K) = (1024, 1024) and (1000, 5), %ld nodes, acts at T = 0, 0.5, 1\n", SIMS, nodes);
    return 0;
}
