// options.cpp -- defaults, environment overrides and range check of emme_options_t (options.hpp)
#include "options.hpp"

#include <cstdlib>

namespace emme {

bool wants_tiled(const emme_params_t& p, bool folded, int fill) {
    const bool shape = p.integration_start_points == 15 || p.integration_start_points == 31;
    return shape && folded && p.integration_accuracy >= 1e-9 && fill == EMME_FILL_AUTO;
}

void options_default(emme_options_t& o) {
    o = emme_options_t{};
    o.size = (int)sizeof(emme_options_t);
    o.node_cache_gb = 176.0;  // both contour classes together (MI355X: 288 GB of HBM3E)
    o.cache_min_batch = 8;
    o.cache_min_depth = 0;
    o.fill = EMME_FILL_AUTO;
    o.phase_table = 1;
    o.em_shared = 1;
    o.wl_min = 4;
    o.union_sel = 2;
    o.union_ipg_few = 2, o.union_few_chunks = 3;
    o.coop_wide_min = 4096;
    o.defer_one_group = 0;
    o.dense_min_cols = 3;
    o.dense_min_tasks = 2000;
    o.dense_cost_ratio = 4.0;
    o.dense_wide = 0;
    o.skip_lost = 1;
    o.lu_split = 0;
    o.lu_group_min_n = 256;
    o.lu_spin_limit = 16000000;  // about 4 s
    o.lu_unblocked = 0;
    o.deriv_cached = 0;
    o.tile_uncached = 0;
    o.dense_stage = 1;
}

void options_env_overrides(emme_options_t& o) {
    auto geti = [](const char* name, int& v) {
        if (const char* e = std::getenv(name)) v = std::atoi(e);
    };
    auto getd = [](const char* name, double& v) {
        if (const char* e = std::getenv(name)) v = std::atof(e);
    };
    getd("EMME_NODE_CACHE_GB", o.node_cache_gb);
    geti("EMME_CACHE_MIN_BATCH", o.cache_min_batch);
    geti("EMME_CACHE_MIN_DEPTH", o.cache_min_depth);
    if (const char* e = std::getenv("EMME_DENSE"))
        if (std::atoi(e) == 0 && o.fill == EMME_FILL_AUTO) o.fill = EMME_FILL_UNION;
    if (const char* e = std::getenv("EMME_UNION"))
        if (std::atoi(e) == 0) o.fill = EMME_FILL_LANES;
    geti("EMME_PHASE_TABLE", o.phase_table);
    geti("EMME_EM_SHARED", o.em_shared);
    geti("EMME_WL_MIN", o.wl_min);
    geti("EMME_UNION_SEL", o.union_sel);
    geti("EMME_UNION_IPG_FEW", o.union_ipg_few);
    geti("EMME_UNION_FEW_CHUNKS", o.union_few_chunks);
    geti("EMME_COOP_WIDE_MIN", o.coop_wide_min);
    if (std::getenv("EMME_DEFER_ONE_GROUP")) o.defer_one_group = 1;
    geti("EMME_DENSE_MIN_COLS", o.dense_min_cols);
    geti("EMME_DENSE_MIN_TASKS", o.dense_min_tasks);
    getd("EMME_DENSE_COST_RATIO", o.dense_cost_ratio);
    geti("EMME_DENSE_WIDE", o.dense_wide);
    geti("EMME_SKIP_LOST", o.skip_lost);
    geti("EMME_LU_SPLIT", o.lu_split);
    if (const char* e = std::getenv("EMME_LU_GROUP")) o.lu_group_min_n = std::atoi(e) <= 0 ? -1 : std::atoi(e);
    geti("EMME_LU_SPIN_LIMIT", o.lu_spin_limit);
    if (std::getenv("EMME_LU_UNBLOCKED")) o.lu_unblocked = 1;
    geti("EMME_DERIV_CACHED", o.deriv_cached);
    geti("EMME_TILE_UNCACHED", o.tile_uncached);
    geti("EMME_DENSE_STAGE", o.dense_stage);
}

int options_check(const emme_options_t* o) {
    if (o->size != (int)sizeof(emme_options_t)) {
        set_error("emme_options_t: size field does not match this library (use emme_options_default)");
        return EMME_EINVAL;
    }
    if (!(o->node_cache_gb >= 0.0) || o->cache_min_batch < 1 || o->cache_min_depth < 0 || o->fill < EMME_FILL_AUTO ||
        o->fill > EMME_FILL_LANES || o->wl_min < 1 || (o->union_sel != 1 && o->union_sel != 2 && o->union_sel != 4) ||
        o->union_ipg_few < 1 || o->union_few_chunks < 0 || o->coop_wide_min < -1 || o->dense_min_cols < 1 ||
        o->dense_min_cols > 17 || o->dense_min_tasks < 0 || !(o->dense_cost_ratio > 0.0) || o->lu_split < 0 ||
        o->lu_split > 16 || o->lu_spin_limit < 1 || o->deriv_cached < 0 || o->deriv_cached > 1 ||
        o->tile_uncached < 0 || o->tile_uncached > 1 || o->dense_stage < 0 || o->dense_stage > 1) {
        set_error("emme_options_t: value out of range");
        return EMME_EINVAL;
    }
    return EMME_OK;
}

}  // namespace emme
