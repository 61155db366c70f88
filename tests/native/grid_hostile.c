/*
 * grid_hostile.c - the grid oracle on scenes whose obstacles, ego, goal or grid origin are not finite or lie far outside the
 * range of int ("Values outside the grid's range").  A stand-alone program: tests/test_grid_hostile.py builds it
 * together with the oracle's sources under -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover and runs it on the
 * case list of tests/hostile_scenes.py, so a conversion of an out-of-range double or a signed overflow anywhere on the way
 * ends the run with a non-zero status.
 *
 * Input (argv[1]), little endian: int32 n_cases, then per case
 *   int32 cfg_bytes, in_bytes, state_bytes, lane_bytes, attr_bytes, ref_bytes, n_obs, ticks
 *   PlannerConfig, SceneIn, SceneState, lane pool, lane attribute pool, reference pool, n_obs ObPoint, n_obs ObMotion.
 * Per case it runs orc_cell_of on the ego and the goal, orc_rasterise and orc_rasterise_bruteforce on the effective obstacles of
 * every tick (the two grids must be equal: exit 3), and `ticks` whole oracle ticks.  Output: one line per case and tick,
 *   case <i> tick <t> start <cell> goal <cell> occupied <n> status <s> expanded <n> digest <hex>
 * which the test compares with the Python models.
 */
#include "../../oracle/dmpp_oracle.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static void* take(FILE* f, size_t n)
{
    void* p = malloc(n ? n : 1);
    if (!p || (n && fread(p, 1, n, f) != n)) { fprintf(stderr, "grid_hostile: short read\n"); exit(2); }
    return p;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: grid_hostile CASES\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    for (int i = 0; i < n_cases; i++) {
        int32_t h[8];
        if (fread(h, 4, 8, f) != 8) return 2;
        if (h[0] != (int32_t)sizeof(PlannerConfig) || h[1] != (int32_t)sizeof(SceneIn) || h[2] != (int32_t)sizeof(SceneState)) {
            fprintf(stderr, "grid_hostile: record sizes %d %d %d differ from the headers' %zu %zu %zu\n", h[0], h[1], h[2],
                    sizeof(PlannerConfig), sizeof(SceneIn), sizeof(SceneState));
            return 2;
        }
        PlannerConfig* c = (PlannerConfig*)take(f, (size_t)h[0]);
        SceneIn* in = (SceneIn*)take(f, (size_t)h[1]);
        SceneState* st = (SceneState*)take(f, (size_t)h[2]);
        GlobalPoint3D* lanes = (GlobalPoint3D*)take(f, (size_t)h[3]);
        uint8_t* attr = (uint8_t*)take(f, (size_t)h[4]);
        GlobalPoint2D* ref = (GlobalPoint2D*)take(f, (size_t)h[5]);
        const int m = h[6], ticks = h[7];
        ObPoint* obs = (ObPoint*)take(f, sizeof(ObPoint) * (size_t)m);
        ObMotion* mot = (ObMotion*)take(f, sizeof(ObMotion) * (size_t)m);
        const size_t cells = (size_t)c->grid_w * (size_t)c->grid_h;
        uint8_t* g0 = (uint8_t*)malloc(cells);
        uint8_t* g1 = (uint8_t*)malloc(cells);
        uint8_t* g2 = (uint8_t*)malloc(cells);
        ObPoint* eff = (ObPoint*)malloc(sizeof(ObPoint) * (size_t)(m ? m : 1));
        int32_t* path = (int32_t*)malloc(sizeof(int32_t) * (size_t)c->max_path);
        for (int t = 0; t < ticks; t++) {
            const int tick = (int)st->tick;
            orc_effective_obstacles(c, obs + in->obs_off, mot + in->obs_off, in->obs_n, tick, eff);
            orc_rasterise(c, in->grid_origin, eff, in->obs_n, g0);
            orc_rasterise_bruteforce(c, in->grid_origin, eff, in->obs_n, g1);
            if (memcmp(g0, g1, cells) != 0) { fprintf(stderr, "grid_hostile: case %d tick %d: rasterise differs from brute force\n", i, t); return 3; }
            size_t occ = 0;
            for (size_t k = 0; k < cells; k++) occ += g1[k];
            const int sc = orc_cell_of(c, in->grid_origin, in->loc.globalpoint.x, in->loc.globalpoint.y);
            const int gc = orc_cell_of(c, in->grid_origin, in->goal.x, in->goal.y);
            PlanOut po; GridOut go;
            memset(&po, 0, sizeof(po)); memset(&go, 0, sizeof(go));
            orc_plan_tick(c, in, lanes, h[4] ? attr : NULL, ref, obs, mot, st, &po, &go, g2, NULL, 0, path, c->max_path);
            if (memcmp(g2, g1, cells) != 0) { fprintf(stderr, "grid_hostile: case %d tick %d: the tick's grid differs from brute force\n", i, t); return 3; }
            if (go.start_cell != sc || go.goal_cell != gc) { fprintf(stderr, "grid_hostile: case %d tick %d: start / goal cell\n", i, t); return 3; }
            printf("case %d tick %d start %d goal %d occupied %zu status %d expanded %d digest %llx\n", i, t, sc, gc, occ, (int)go.status,
                   (int)go.n_expanded, (unsigned long long)go.order_digest);
        }
        free(path); free(eff); free(g2); free(g1); free(g0);
        free(mot); free(obs); free(ref); free(attr); free(lanes); free(st); free(in); free(c);
    }
    fclose(f);
    printf("grid_hostile ok: %d cases\n", (int)n_cases);
    return 0;
}
