// hh_tune / hh_tune_get: the one table of the library's tuning knobs.  A row
// names the key, the variable it stores into (declared once, in the header of
// the code that reads it), the values it accepts and what it does.  A value is
// accepted when it is one of `also`, or lies in [lo, hi] and, with a step, is a
// multiple of it.  Two keys are not a plain store and are handled by name in
// hh_tune / hh_tune_get: sweep_trace (owns a device buffer) and
// twostep_budget_mb (kept in bytes); upper_tiles 1 also needs its build.
#include <climits>

#include "ice_internal.hpp"

namespace hh {
namespace {

struct Knob {
    const char* name;
    int* vi;        // the variable: an int ...
    int64_t* vl;    // ... or an int64_t (both null: a key with a setter of its own)
    int64_t lo, hi, step;
    int n_also;
    int64_t also[5];
    const char* doc;
};

Knob range(const char* name, int* v, int64_t lo, int64_t hi, const char* doc) {
    return Knob{name, v, nullptr, lo, hi, 0, 0, {}, doc};
}
Knob range(const char* name, int64_t* v, int64_t lo, int64_t hi, const char* doc) {
    return Knob{name, nullptr, v, lo, hi, 0, 0, {}, doc};
}
// the values of `set` alone (an empty range)
Knob set_of(const char* name, int* v, std::initializer_list<int64_t> set, const char* doc) {
    Knob k{name, v, nullptr, 1, 0, 0, 0, {}, doc};
    for (int64_t x : set) k.also[k.n_also++] = x;
    return k;
}

const Knob kKnobs[] = {
    // -- matrix layout: read when a matrix is built, no effect on one that exists
    Knob{"band_w", nullptr, &g_band_w, 0, kBandMaxW, 16, 1, {-1}, "uint8 band half-width: -1 auto, 0 off, else forced"},
    range("band4", &g_band4, 0, 1, "nibble band beyond the uint8 band"),
    range("band_cis", &g_band_cis, 0, 1, "the bands hold cis pixels only (0: by diagonal and count alone)"),
    range("flat_max", &g_flat_max, 0, 255, "longest row (uint4) of a flat tile segment, 0: no flat tiles"),
    range("flat_cols", &g_flat_cols, -1, 1, "flat tiles swept by column group: -1 auto, 0, 1"),
    range("flat_group", &g_flat_group, 0, 256, "flat tiles per column group, 0: auto (11 .. 44)"),
    Knob{"unit_entries", nullptr, &g_unit_entries, 4096, 1 << 24, 0, 1, {0}, "payload words per work unit, 0: auto"},
    range("upper_tiles", &g_upper_tiles, -1, 1, "upper-triangle tiles: -1 auto, 0, 1 (the 4096-column build only)"),
    range("host_build", &g_host_build, 0, 1, "1: the host builder for every pixel table"),
    range("build_debug", &g_build_debug, 0, 9, "build and balance phase times on stderr"),
    // -- ICE sweep: read at every sweep (uband at hh_ice_create)
    set_of("flatw_pipe", &g_flatw_pipe, {0, 2, 3}, "k_sweep_flatw: 0 no prefetch, 2 masked prefetch, 3 raw prefetch"),
    set_of("flatw_waves", &g_flatw_waves, {8, 10, 11}, "waves per k_sweep_flatw block"),
    set_of("flatw_waves_up", &g_flatw_waves_up, {8, 11}, "the same for the column-side kernel"),
    range("flat_defer", &g_flat_defer, 0, 1, "k_sweep_flat merges a tile's sums after the next tile's barrier"),
    range("tiled_pf", &g_tiled_pf, 0, 2, "k_sweep_tiled: 0 plain loops, 1 pipelined loads, 2 and rows reduced in turn"),
    set_of("band_rows", &g_band_rows, {0, 64, 128, 256}, "rows per band block, 0: auto"),
    range("band_fused", &g_band_fused, 0, 1, "the band segments in one launch"),
    range("band_concurrent", &g_band_concurrent, 0, 1, "the band sweep on a side stream"),
    range("split_tiles", &g_split_tiles, 0, 1, "with band_concurrent: the tiled kernel on a second side stream"),
    range("conc_order", &g_conc_order, 0, 2, "three-stream launch order"),
    range("conc_min_bytes", &g_conc_min_bytes, 0, INT64_MAX, "payload from which the sweep forks into streams"),
    range("sweep_sched", &g_sweep_sched, -1, 2, "sweep schedule: -1 auto, 0 one stream, 1 all concurrent, 2 flat alone then tiled beside band"),
    range("uband", &g_uband, 0, 2, "upper-band sweep: 0 off, 1 auto, 2 always"),
    range("ub_skip", &g_ub_skip, 0, 1, "upper-band sweep leaves out the dead rectangles"),
    range("ub_xcd", &g_ub_xcd, 0, 1, "upper-band blocks in contiguous ranges per XCD"),
    range("ub_fast", &g_ub_fast, 0, 1, "upper-band walk on exponent-zero operands"),
    range("sweep_single", &g_sweep_single, -1, 1, "the whole sweep in one launch: -1 auto, 0, 1"),
    range("iter_events", &g_iter_events, 0, 1, "hh_ice_run: HIP events around every sweep"),
    range("fuse_stats", &g_fuse_stats, -1, 2, "stats mode: -1 auto, 0 unfused, 1 small, 2 big (changes results)"),
    Knob{"sweep_trace", nullptr, nullptr, 0, INT32_MAX, 0, 0, {}, "block capacity of the one-launch sweep's timeline"},
    // -- compartments / PCA (comp.hip)
    range("pca_method", &g_pca_method, 0, 1, "0 block subspace iteration, 1 block Krylov"),
    range("pca_p", &g_pca_p, 2, 8, "Cor products per Krylov cycle"),
    range("pca_coop", &g_pca_coop, 0, 1, "Krylov orthogonalisation in one launch per product"),
    range("pca_debug", &g_pca_debug, 0, 9, "per-cycle trace on stderr"),
    range("syrk_split", &g_syrk_split, -1, 64, "Cov K splits: -1 auto, 0 never, n forced (changes results)"),
    range("cor_sym", &g_cor_sym, 0, 3, "Krylov Cor products on the upper triangle: 0 full, 1, 2, 3"),
    set_of("ortho_tpb", &g_ortho_tpb, {0, 1, 2, 4, 8}, "k_ortho rows per block / 64, 0: auto"),
    range("ortho_min_tpb", &g_ortho_min_tpb, 1, 2, "the automatic choice's smallest ortho_tpb"),
    range("ortho_lowsync", &g_ortho_lowsync, 0, 1, "k_ortho's Full mode as low-synch CGS2"),
    range("ortho_grid_cap", &g_ortho_grid_cap, 0, 64, "a lower cap on k_ortho's grid, 0: none"),
    range("ortho_abort_test", &g_ortho_abort_test, 0, 2, "act as if k_ortho's barrier timed out (tests)"),
    // -- two-step correction (dense.hip)
    Knob{"symvc_rows", &g_symvc_rows, nullptr, 16, 1024, 16, 0, {}, "rows per k_ts_gemv block"},
    range("symvc_out", &g_symvc_out, 0, 1, "pass 3 with one LDS tile"),
    range("symvc_stream", &g_symvc_stream, 0, 1, "passes 1-2 as row-streaming GEMVs"),
    range("twostep_devglue", &g_twostep_devglue, 0, 1, "gap / alpha glue on the device"),
    Knob{"twostep_budget_mb", nullptr, nullptr, 0, INT64_MAX >> 20, 0, 0, {}, "hh_twostep_batch workspace, 0: free HBM"},
    // -- pairs, loops, coarsen, saddle, pileup, scc, trans, transeig, coverage: read by the next call
    range("parse_ablate", &g_parse_ablate, 0, 3, "pair parser timing ablations (wrong results while set)"),
    range("rank_lds_buckets", &g_rank_lds_buckets, 0, 8192, "hh_diag_rank_pixels: LDS buckets per block"),
    range("coarsen_tile", &g_coarsen_tile, 64, HH_COARSEN_TILE, "coarse columns per work item"),
    range("saddle_diag_tile", &g_saddle_diag_tile, 64, HH_SADDLE_DIAG_TILE, "diagonals per wave of the expected sums"),
    range("pileup_chunk", &g_pileup_chunk, 1, HH_PILEUP_CHUNK, "features per chunk of the pileup sums (changes results)"),
    Knob{"scc_rows", &g_scc_rows, nullptr, 4, 32, 4, 1, {0}, "rows per work item of the stratum moments, 0: from h (changes results)"},
    range("trans_trips", &g_trans_trips, 1, HH_TRANS_MAX_TRIPS, "trips of 64 pixels per span of the trans block sums (changes results)"),
    range("teig_rows", &g_teig_rows, 1, HH_TEIG_MAX_ROWS, "rows (waves) per block of the trans operator's product"),
    range("cov_rows", &g_cov_rows, 1, HH_COV_MAX_ROWS, "bins (waves) per block of the coverage walk"),
};

const Knob* find(const std::string& key) {
    for (const Knob& k : kKnobs)
        if (key == k.name) return &k;
    HH_THROW(HH_ERR_ARG, "unknown tuning key " + key);
}

bool legal(const Knob& k, int64_t v) {
    for (int i = 0; i < k.n_also; ++i)
        if (v == k.also[i]) return true;
    return v >= k.lo && v <= k.hi && (k.step == 0 || v % k.step == 0);
}

// "key = allowed values (what it does)" for the error text
std::string allowed(const Knob& k) {
    std::string s = std::string(k.name) + " = ";
    auto num = [](int64_t x) { return x == INT64_MAX ? std::string("2^63 - 1") : std::to_string(x); };
    const char* sep = "";
    if (k.n_also) {
        s += "{";
        for (int i = 0; i < k.n_also; ++i, sep = ", ") s += sep + num(k.also[i]);
        s += "}";
        sep = " or ";
    }
    if (k.lo <= k.hi) {
        s += std::string(sep) + "[" + num(k.lo) + ", " + num(k.hi) + "]";
        if (k.step) s += " in steps of " + num(k.step);
    }
    return s + " (" + k.doc + ")";
}

// the keys that are not a plain store
void set_sweep_trace(int64_t value) {
    if (g_trace) HIP_CHECK(hipFree(g_trace));
    g_trace = nullptr;
    g_trace_cap = g_trace_n = 0;
    if (value) HIP_CHECK(hipMalloc(&g_trace, (size_t)value * 3 * sizeof(unsigned long long)));
    g_trace_cap = value;
}

}  // namespace
}  // namespace hh

using namespace hh;

extern "C" {

int hh_tune(const char* key, int64_t value) {
    return guard([&] {
        HH_REQUIRE(key, "null key");
        const Knob& k = *find(key);
        HH_REQUIRE(legal(k, value), "allowed: " + allowed(k) + ", got " + std::to_string(value));
        const std::string name(k.name);
        if (name == "upper_tiles")
            HH_REQUIRE(kUpperBuild || value != 1,
                       "upper_tiles: upper-triangle tiles need the 4096-column build (libhichap_hip_up.so, "
                       "-DHH_KWBITS=12)");
        if (name == "sweep_trace") set_sweep_trace(value);
        else if (name == "twostep_budget_mb") g_twostep_budget = value << 20;  // kept in bytes
        else if (k.vi) *k.vi = (int)value;
        else *k.vl = value;
    });
}

int hh_tune_get(const char* key, int64_t* value) {
    return guard([&] {
        HH_REQUIRE(key && value, "null");
        const Knob& k = *find(key);
        const std::string name(k.name);
        if (name == "sweep_trace") *value = g_trace_cap;
        else if (name == "twostep_budget_mb") *value = g_twostep_budget >> 20;
        else *value = k.vi ? (int64_t)*k.vi : *k.vl;
    });
}

}  // extern "C"
