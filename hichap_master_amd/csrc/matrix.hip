// Contact-matrix construction in HBM: cooler pixel table -> tiled pixel
// layout (ice_internal.hpp): tile/unit planning shared with the
// on-device generator (synth.hip), host fill + upload, and export for checks.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cmath>
#include <numeric>
#include <exception>
#include <mutex>
#include <thread>

#include "ice_internal.hpp"

namespace hh {

static thread_local std::string g_last_error;
bool flat_cols_on(int32_t nJ) { return g_flat_cols > 0 || (g_flat_cols < 0 && nJ >= 32); }
bool upper_tiles_on(int32_t nJ) {
    return kUpperBuild && (g_upper_tiles > 0 || (g_upper_tiles < 0 && flat_cols_on(nJ)));
}
// payload-word equivalent of one tile's fixed cost in the unit split (C4 shard 8/8: 0.79 -> 0.65 ms/iter)
constexpr int64_t kTileCost = 32768;
// the nibble band's edges (ice_internal.hpp): occupancy break-even of 4-bit slots vs 2-byte tile
// entries, and the share of a diagonal's pixels with count > 15 from which the uint8 band keeps it
constexpr double kBand4Density = 0.25;
constexpr double kBand8Big = 0.05;

int32_t choose_band_w(const std::vector<double>& occ, int ignore_diags) {
    if (g_band_w >= 0) return (int32_t)std::min<int64_t>(g_band_w, kBandMaxW) & ~15;
    int64_t d = std::max(1, ignore_diags);
    if (d > 1) return 0;  // diagonal 1 dropped: no dense neighbourhood to exploit
    while (d < (int64_t)occ.size() && occ[d] >= kBandDensity) ++d;
    return (int32_t)((d - 1) & ~15LL);
}

BandWidths choose_band_widths(const std::vector<double>& occ, const std::vector<double>& big, int ignore_diags) {
    BandWidths bw;
    bw.w8 = bw.w4 = choose_band_w(occ, ignore_diags);
    if (g_band_w >= 0 || !g_band4 || std::max(1, ignore_diags) > 1) return bw;
    // outer edge: occupancy >= kBand4Density from diagonal 1 on
    int64_t d4 = 1;
    while (d4 < (int64_t)occ.size() && occ[d4] >= kBand4Density) ++d4;
    --d4;
    // inner edge: past the last diagonal where counts > 15 are common
    int64_t d8 = 0;
    for (int64_t d = 1; d <= d4 && d < (int64_t)big.size(); ++d)
        if (big[d] >= kBand8Big) d8 = d;
    int64_t w8 = (d8 + 15) & ~15LL;
    if (w8 > bw.w8) w8 = bw.w8;  // no uint8 slots below their own break-even
    const int64_t k = (d4 - w8) & ~31LL;
    if (k < 32) return bw;       // no nibble band: the uint8 band as before
    bw.w8 = (int32_t)w8;
    bw.w4 = (int32_t)(w8 + k);
    return bw;
}
void set_error(const std::string& msg) { g_last_error = msg; }

namespace {
// The tiles of one row-block (plan_tiles' per-block work, entry offsets
// relative to the block's first tile).
struct BlockTiles {
    std::vector<int32_t> J;
    std::vector<int64_t> ent, entn;
    std::vector<uint32_t> rp, rpn, fw;
    std::vector<uint16_t> perm, band, frec;
    std::vector<int32_t> frec_of;  // per tile: flat record index within the block, -1
    std::vector<uint8_t> flat;
    int64_t ent_total = 0, entn_total = 0;
};

// fn(0 .. n-1) on nt host threads (work-stealing counter); the first
// exception any thread throws stops the others and is rethrown here after
// the join, so it reaches guard() as an error code instead of
// std::terminate (a throwing std::thread body).
template <class F>
static void parallel_blocks(int nt, int64_t n, F&& fn) {
    std::atomic<int64_t> next{0};
    std::exception_ptr err;
    std::mutex mu;
    auto work = [&] {
        try {
            for (int64_t i; (i = next.fetch_add(1)) < n;) fn(i);
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu);
            if (!err) err = std::current_exception();
            next.store(n);
        }
    };
    std::vector<std::thread> th;
    try {
        for (int t = 1; t < nt; ++t) th.emplace_back(work);
    } catch (...) {  // thread creation failed: run on fewer threads
    }
    work();
    for (auto& t : th) t.join();
    if (err) std::rethrow_exception(err);
}

void plan_block(const uint16_t* cntw, const uint16_t* cntn, int64_t nloc, int32_t nJ, int64_t rb, BlockTiles& B) {
    std::vector<uint32_t> rp(kR + 1), rpn(kR + 1);
    const int64_t r0 = rb * kR, r1 = std::min<int64_t>(nloc, r0 + kR);
    // the block's counts transposed to tile-major (one pass over its rows)
    std::vector<uint16_t> tw((size_t)nJ * kR, 0), tn((size_t)nJ * kR, 0);
    for (int64_t r = r0; r < r1; ++r)
        for (int32_t J = 0; J < nJ; ++J) {
            tw[(size_t)J * kR + (r - r0)] = cntw[r * nJ + J];
            if (cntn) tn[(size_t)J * kR + (r - r0)] = cntn[r * nJ + J];
        }
    int64_t ent = 0, entn = 0;
    for (int32_t J = 0; J < nJ; ++J) {
        const uint16_t* cw_ = &tw[(size_t)J * kR];
        const uint16_t* cn_ = &tn[(size_t)J * kR];
        rp[0] = rpn[0] = 0;
        for (int k = 0; k < kR; ++k) {
            rp[k + 1] = rp[k] + (uint32_t)pad4(cw_[k]);
            rpn[k + 1] = rpn[k] + (uint32_t)pad8(cn_[k]);
        }
        if (rp[kR] == 0 && rpn[kR] == 0) continue;
        B.J.push_back(J);
        B.ent.push_back(ent);
        B.entn.push_back(entn);
        B.rp.insert(B.rp.end(), rp.begin(), rp.end());
        B.rpn.insert(B.rpn.end(), rpn.begin(), rpn.end());
        // per segment (narrow first): rows by decreasing length (uint4
        // count, counting sort on min(len, 255), stable) and the bands of
        // that order; a tile whose nonempty segments have only short rows
        // (<= g_flat_max uint4) is *flat*: its perms list the nonempty rows
        // in row order instead (band[kFlatFlag] = 1, band[kFlatRows] = count)
        uint16_t perm[2][kR];
        uint16_t band[2][kBandSlots] = {{0}};
        uint32_t maxlen[2];
        for (int seg = 0; seg < 2; ++seg) {
            const std::vector<uint32_t>& q = seg == 0 ? rpn : rp;
            const int sh = seg == 0 ? 3 : 2;
            uint32_t key[kR];
            int hist[257] = {0};
            for (int k = 0; k < kR; ++k) {
                const uint32_t len = (q[k + 1] - q[k]) >> sh;
                key[k] = 255u - std::min<uint32_t>(len, 255u);  // descending
                ++hist[key[k] + 1];
            }
            for (int k = 0; k < 256; ++k) hist[k + 1] += hist[k];
            for (int k = 0; k < kR; ++k) perm[seg][hist[key[k]]++] = (uint16_t)k;
            int pos = 0;
            for (int g = 0; g < kBands; ++g) {
                while (pos < kR && ((q[perm[seg][pos] + 1] - q[perm[seg][pos]]) >> sh) >= band_min(g)) ++pos;
                band[seg][g + 1] = (uint16_t)pos;
            }
            maxlen[seg] = 255u - key[perm[seg][0]];
        }
        const bool flat = g_flat_max > 0 && maxlen[0] <= (uint32_t)g_flat_max &&
                          maxlen[1] <= (uint32_t)g_flat_max && (rpn[kR] >> 3) < 65536u && (rp[kR] >> 2) < 65536u;
        uint32_t fw[kFlatMeta] = {0};
        if (flat) {
            for (int seg = 0; seg < 2; ++seg) {
                const std::vector<uint32_t>& q = seg == 0 ? rpn : rp;
                const int sh = seg == 0 ? 3 : 2;
                int nfr = 0;
                uint32_t st[kR + 1];  // uint4 starts of the nonempty rows, then the end
                for (int k = 0; k < kR; ++k)
                    if (q[k + 1] > q[k]) {
                        st[nfr] = q[k] >> sh;
                        perm[seg][nfr++] = (uint16_t)k;
                    }
                for (int k = nfr; k < kR; ++k) perm[seg][k] = 0;
                const uint32_t Q = q[kR] >> sh;
                st[nfr] = Q;
                band[seg][kFlatFlag] = nfr > 0 ? 1 : 0;
                band[seg][kFlatRows] = (uint16_t)nfr;
                // wave w takes the rows starting in [Q w / 8, Q (w + 1) / 8);
                // with the column-grouped sweep one wave walks the whole tile
                // (k_sweep_flatw), and the one-launch sweep's flat body must
                // sum each row in that same order: wave 0 takes every row
                uint32_t* f = fw + seg * 2 * (kFlatWaves + 1);
                for (int w = 0; w <= kFlatWaves; ++w) {
                    const uint32_t tq = flat_cols_on(nJ) ? (w == 0 ? 0u : Q) : (uint32_t)(((uint64_t)Q * w) / kFlatWaves);
                    const int i = (int)(std::lower_bound(st, st + nfr, tq) - st);
                    f[2 * w] = st[i];
                    f[2 * w + 1] = (uint32_t)i;
                }
            }
        }
        B.fw.insert(B.fw.end(), fw, fw + kFlatMeta);
        if (flat) {
            B.frec_of.push_back((int32_t)(B.frec.size() / (kFrecU4 * 8)));
            const size_t base = B.frec.size();
            B.frec.resize(base + kFrecU4 * 8, 0);
            uint16_t* rec = &B.frec[base];
            for (int seg = 0; seg < 2; ++seg) {
                const std::vector<uint32_t>& q = seg == 0 ? rpn : rp;
                const int sh = seg == 0 ? 3 : 2;
                const int nfr = band[seg][kFlatRows];
                uint16_t* st = rec + seg * (kR + 1);
                uint16_t* id = rec + 2 * (kR + 1) + seg * kR;
                for (int i = 0; i <= kR; ++i) st[i] = (uint16_t)(i < nfr ? q[perm[seg][i]] >> sh : q[kR] >> sh);
                for (int i = 0; i < kR; ++i) id[i] = perm[seg][i];
            }
        } else {
            B.frec_of.push_back(-1);
        }
        B.flat.push_back(flat ? 1 : 0);
        for (int seg = 0; seg < 2; ++seg) {
            B.perm.insert(B.perm.end(), perm[seg], perm[seg] + kR);
            B.band.insert(B.band.end(), band[seg], band[seg] + kBandSlots);
        }
        ent += rp[kR];
        entn += rpn[kR];
    }
    B.ent_total = ent;
    B.entn_total = entn;
}
}  // namespace

TilePlan plan_tiles(const uint16_t* cntw, const uint16_t* cntn, int64_t nloc, int32_t nJ,
                    const std::vector<uint16_t>& row_group, int64_t row_lo, bool upper) {
    TilePlan P;
    P.nloc = nloc;
    P.nJ = nJ;
    P.upper = upper ? 1 : 0;
    P.row_lo = row_lo;
    P.nrb = (nloc + kR - 1) / kR;
    P.tile_of.assign((size_t)P.nrb * nJ, -1);
    P.blk_tile_ptr.assign(P.nrb + 1, 0);
    P.blk_unit_ptr.assign(P.nrb + 1, 0);
    // row-blocks planned in parallel (independent), concatenated in order:
    // the plan is identical to the serial one
    std::vector<BlockTiles> blocks((size_t)P.nrb);
    const auto tp0 = std::chrono::steady_clock::now();
    {
        const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::thread::hardware_concurrency(),
                                                                     (int64_t)16, P.nrb}));
        parallel_blocks(nt, P.nrb, [&](int64_t rb) { plan_block(cntw, cntn, nloc, nJ, rb, blocks[rb]); });
    }
    const auto tp1 = std::chrono::steady_clock::now();
    // concatenation in block order.  Its cost was first-touch page faults of
    // the ~6 KB per tile of plan arrays (45 ms at 22 572 tiles, a parallel
    // copy into 4 KiB pages no faster): the big arrays now live on
    // THP-advised mappings (HVec), are sized without being touched, and the
    // blocks are copied into them by the planning threads.
    size_t nt_all = 0, nfrec = 0;
    std::vector<size_t> t_off((size_t)P.nrb + 1, 0), f_off((size_t)P.nrb + 1, 0);
    for (int64_t rb = 0; rb < P.nrb; ++rb) {
        const BlockTiles& B = blocks[rb];
        const size_t k = B.J.size();
        if (B.rp.size() != k * (kR + 1) || B.rpn.size() != k * (kR + 1) || B.fw.size() != k * kFlatMeta ||
            B.perm.size() != k * 2 * kR || B.band.size() != k * 2 * kBandSlots || B.flat.size() != k)
            HH_THROW(HH_ERR_STATE, "tile plan: inconsistent per-block array sizes");
        t_off[rb] = nt_all;
        f_off[rb] = nfrec;
        nt_all += k;
        nfrec += B.frec.size();
    }
    t_off[P.nrb] = nt_all;
    f_off[P.nrb] = nfrec;
    P.tile_J.reserve(nt_all);
    P.tile_ent.reserve(nt_all);
    P.tile_entn.reserve(nt_all);
    P.tile_rb.reserve(nt_all);
    P.tile_frec.reserve(nt_all);
    P.tile_flat.reserve(nt_all);
    P.tile_rp.resize(nt_all * (kR + 1));
    P.tile_rpn.resize(nt_all * (kR + 1));
    P.tile_fw.resize(nt_all * kFlatMeta);
    P.tile_perm.resize(nt_all * 2 * kR);
    P.tile_band.resize(nt_all * 2 * kBandSlots);
    P.frec.resize(nfrec);
    {
        const int nt = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::thread::hardware_concurrency(),
                                                                     (int64_t)16, P.nrb}));
        parallel_blocks(nt, P.nrb, [&](int64_t rb) {
                const BlockTiles& B = blocks[rb];
                const size_t t0 = t_off[rb];
                std::copy(B.rp.begin(), B.rp.end(), P.tile_rp.begin() + t0 * (kR + 1));
                std::copy(B.rpn.begin(), B.rpn.end(), P.tile_rpn.begin() + t0 * (kR + 1));
                std::copy(B.fw.begin(), B.fw.end(), P.tile_fw.begin() + t0 * kFlatMeta);
                std::copy(B.perm.begin(), B.perm.end(), P.tile_perm.begin() + t0 * 2 * kR);
                std::copy(B.band.begin(), B.band.end(), P.tile_band.begin() + t0 * 2 * kBandSlots);
                std::copy(B.frec.begin(), B.frec.end(), P.frec.begin() + f_off[rb]);
        });
    }
    int64_t ent = 0, entn = 0;
    for (int64_t rb = 0; rb < P.nrb; ++rb) {
        BlockTiles& B = blocks[rb];
        P.blk_tile_ptr[rb] = (int32_t)P.tile_J.size();
        const int32_t frec0 = (int32_t)(f_off[rb] / (kFrecU4 * 8));
        for (size_t i = 0; i < B.J.size(); ++i) {
            P.tile_of[rb * nJ + B.J[i]] = (int32_t)P.tile_J.size();
            P.tile_J.push_back(B.J[i]);
            P.tile_ent.push_back(ent + B.ent[i]);
            P.tile_entn.push_back(entn + B.entn[i]);
            P.tile_rb.push_back((int32_t)rb);
            P.tile_frec.push_back(B.frec_of[i] < 0 ? -1 : frec0 + B.frec_of[i]);
        }
        P.tile_flat.insert(P.tile_flat.end(), B.flat.begin(), B.flat.end());
        ent += B.ent_total;
        entn += B.entn_total;
        B = BlockTiles();  // free as we go
    }
    P.blk_tile_ptr[P.nrb] = (int32_t)P.tile_J.size();
    if (g_build_debug)
        fprintf(stderr, "[plan] %zu tiles: blocks %.3f ms, concat %.3f ms\n", nt_all,
                std::chrono::duration<double, std::milli>(tp1 - tp0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp1).count());
    P.n_entries_padded = ent;
    P.n_narrow_padded = entn;
    // units: ~4 MiB of payload each on big matrices (measured best on C4),
    // but at least ~4096 units so small matrices still fill 256 CUs.
    // Sizes in 4-byte payload words (a narrow entry is half a word).
    const int64_t words = ent + entn / 2;
    const int64_t unit_cap = g_unit_entries > 0 ? g_unit_entries
                                                : std::max<int64_t>(1 << 15, std::min<int64_t>(1 << 20, words / 4096));
    // the per-tile cost only where the units are small (shards, single
    // chromosomes, C3, C4 shards): on the whole C4 matrix (unit cap 446 K
    // words) it changes no time but splits the flat units 3x, and each unit
    // re-stages its bias slices (flat-kernel PMC traffic 7.05 -> 7.96 GB per
    // sweep, profiles/r2_tile_cost_ab.log for the time)
    const int64_t tile_fixed = unit_cap < (3 << 17) ? kTileCost : 0;
    auto tile_words = [&](int32_t t, int k0, int k1) -> int64_t {
        const uint32_t* a = &P.tile_rp[(size_t)t * (kR + 1)];
        const uint32_t* b = &P.tile_rpn[(size_t)t * (kR + 1)];
        return (int64_t)(a[k1] - a[k0]) + (int64_t)(b[k1] - b[k0]) / 2;
    };
    auto emit = [&](int64_t rb, int32_t ta, int32_t tb, int32_t rlo, int32_t rhi) {
        const int64_t g0 = rb * kR + rlo, g1 = rb * kR + rhi - 1;
        P.u_tlo.push_back(ta);
        P.u_thi.push_back(tb);
        P.u_rb.push_back((int32_t)rb);
        P.u_rlo.push_back(rlo);
        P.u_rhi.push_back(rhi);
        P.u_slot.push_back((int32_t)P.n_part);
        P.u_whole.push_back(rlo == 0 && rhi == (int32_t)(std::min<int64_t>(nloc, rb * kR + kR) - rb * kR) ? 1 : 0);
        P.u_glo.push_back(row_group[g0]);
        P.u_ghi.push_back(row_group[g1]);
        P.u_flat.push_back(P.u_whole.back() && P.tile_flat[ta] ? 1 : 0);
        P.n_part += rhi - rlo;
    };
    for (int64_t rb = 0; rb < P.nrb; ++rb) {
        P.blk_unit_ptr[rb] = (int32_t)P.u_tlo.size();
        const int32_t nr = (int32_t)(std::min<int64_t>(nloc, rb * kR + kR) - rb * kR);
        const int32_t ta = P.blk_tile_ptr[rb], tb = P.blk_tile_ptr[rb + 1];
        int32_t cur = ta;
        int64_t cur_sz = 0;
        for (int32_t t = ta; t < tb; ++t) {
            // a tile's fixed cost (staging, the per-tile latency chain) counts
            // toward the unit's size: runs of tiny trans tiles stay short
            const int64_t sz = tile_words(t, 0, kR) + tile_fixed;
            if (sz > unit_cap) {
                if (cur < t) emit(rb, cur, t, 0, nr);
                int32_t rlo = 0;
                int64_t acc = 0;
                for (int32_t k = 0; k < nr; ++k) {
                    const int64_t len = tile_words(t, k, k + 1);
                    if (acc > 0 && acc + len > unit_cap) {
                        emit(rb, t, t + 1, rlo, k);
                        rlo = k;
                        acc = 0;
                    }
                    acc += len;
                }
                emit(rb, t, t + 1, rlo, nr);
                cur = t + 1;
                cur_sz = 0;
            } else if (flat_cols_on(nJ) && P.tile_flat[t]) {
                // column-grouped flat sweep: every flat tile its own unit
                if (cur < t) emit(rb, cur, t, 0, nr);
                emit(rb, t, t + 1, 0, nr);
                cur = t + 1;
                cur_sz = 0;
            } else {
                // a unit is all flat tiles or none (two sweep kernels)
                if (cur < t && (cur_sz + sz > unit_cap || P.tile_flat[t] != P.tile_flat[cur])) {
                    emit(rb, cur, t, 0, nr);
                    cur = t;
                    cur_sz = 0;
                }
                cur_sz += sz;
            }
        }
        if (cur < tb) emit(rb, cur, tb, 0, nr);
    }
    P.blk_unit_ptr[P.nrb] = (int32_t)P.u_tlo.size();
    // launch lists: the tiled-kernel units, then the flat-kernel units
    P.n_units_flat = 0;
    for (size_t u = 0; u < P.u_tlo.size(); ++u)
        if (!P.u_flat[u]) P.u_order.push_back((int32_t)u);
    for (size_t u = 0; u < P.u_tlo.size(); ++u)
        if (P.u_flat[u]) {
            P.u_order.push_back((int32_t)u);
            ++P.n_units_flat;
            for (int32_t t = P.u_tlo[u]; t < P.u_thi[u]; ++t) P.payload_bytes_flat += 4 * tile_words(t, 0, kR);
        }
    if (flat_cols_on(nJ) && P.n_units_flat) {
        // flat groups: the flat units ordered by (column tile, row-block), cut
        // into runs of <= g_flat_group with one column tile; groups dispatched
        // by payload, largest first (a group's partials do not depend on it)
        std::vector<int32_t> fu;
        for (size_t u = 0; u < P.u_tlo.size(); ++u)
            if (P.u_flat[u]) fu.push_back((int32_t)u);
        std::stable_sort(fu.begin(), fu.end(), [&](int32_t a, int32_t b) {
            const int32_t ja = P.tile_J[P.u_tlo[a]], jb = P.tile_J[P.u_tlo[b]];
            return ja != jb ? ja < jb : P.u_rb[a] < P.u_rb[b];
        });
        // (>= ~512 groups: with the three-stream sweep at shard size the
        // other kernels fill the flat launch's tail; N = 8 C4 shards mean
        // 0.542 -> 0.534 ms with 22-tile groups, profiles/r4u_shard_knobs.log)
        const size_t gmax = g_flat_group > 0 ? (size_t)g_flat_group
                                             : std::min<size_t>(44, std::max<size_t>(11, fu.size() / 512));
        std::vector<std::pair<int64_t, std::pair<int32_t, int32_t>>> groups;  // (-words, [lo, hi) in fu)
        for (size_t a = 0; a < fu.size();) {
            size_t e = a;
            int64_t w = 0;
            const int32_t J = P.tile_J[P.u_tlo[fu[a]]];
            while (e < fu.size() && e - a < gmax && P.tile_J[P.u_tlo[fu[e]]] == J) {
                w += tile_words(P.u_tlo[fu[e]], 0, kR);
                ++e;
            }
            groups.push_back({-w, {(int32_t)a, (int32_t)e}});
            a = e;
        }
        std::stable_sort(groups.begin(), groups.end(),
                         [](const auto& x, const auto& y) { return x.first < y.first; });
        P.fg_ptr.assign(1, 0);
        for (const auto& g : groups) {
            for (int32_t k = g.second.first; k < g.second.second; ++k) P.fg_unit.push_back(fu[k]);
            P.fg_ptr.push_back((int32_t)P.fg_unit.size());
        }
        P.fg_desc.reserve(P.fg_unit.size());
        for (int32_t u : P.fg_unit) {
            const int32_t t = P.u_tlo[u];
            const uint32_t* fw = &P.tile_fw[(size_t)t * kFlatMeta];
            const uint32_t* fww = fw + 2 * (kFlatWaves + 1);
            FlatDesc d{};
            d.entn = P.tile_entn[t];
            d.ent = P.tile_ent[t];
            d.frec = P.tile_frec[t];
            d.slot = P.u_slot[u];
            d.qbn = fw[2 * kFlatWaves];
            d.qbw = fww[2 * kFlatWaves];
            d.nr = (uint16_t)P.u_rhi[u];
            d.nfn = (uint16_t)fw[2 * kFlatWaves + 1];
            d.nfw = (uint16_t)fww[2 * kFlatWaves + 1];
            d.glo = P.u_glo[u];
            d.ghi = P.u_ghi[u];
            d.upper = tile_is_upper(P.upper, row_lo, P.u_rb[u], P.tile_J[t]) ? 1 : 0;
            d.rb = (uint32_t)P.u_rb[u];
            P.fg_desc.push_back(d);
        }
    }
    // column slots of the upper tiles' column side: per flat group one (if
    // any of its tiles is strictly upper), per tile of every other unit one;
    // per column tile J the list of its slots in slot order (k_colsum)
    P.u_cslot.assign(P.u_tlo.size(), -1);
    if (P.upper) {
        std::vector<std::vector<int32_t>> byJ((size_t)nJ);
        auto grouped = [&](size_t u) { return flat_cols_on(nJ) && P.u_flat[u]; };
        for (size_t u = 0; u < P.u_tlo.size(); ++u) {
            if (grouped(u)) continue;
            bool any = false;
            for (int32_t t = P.u_tlo[u]; t < P.u_thi[u]; ++t) any |= tile_is_upper(1, row_lo, P.u_rb[u], P.tile_J[t]);
            if (!any) continue;
            P.u_cslot[u] = (int32_t)P.n_cslots;
            for (int32_t t = P.u_tlo[u]; t < P.u_thi[u]; ++t)
                if (tile_is_upper(1, row_lo, P.u_rb[u], P.tile_J[t]))
                    byJ[(size_t)P.tile_J[t]].push_back((int32_t)(P.n_cslots + (t - P.u_tlo[u])));
            P.n_cslots += P.u_thi[u] - P.u_tlo[u];
        }
        const size_t ng = P.fg_ptr.empty() ? 0 : P.fg_ptr.size() - 1;
        P.fg_cslot.assign(ng, -1);
        for (size_t g = 0; g < ng; ++g) {
            bool any = false;
            for (int32_t k = P.fg_ptr[g]; k < P.fg_ptr[g + 1]; ++k) any |= P.fg_desc[k].upper != 0;
            if (!any) continue;
            P.fg_cslot[g] = (int32_t)P.n_cslots;
            byJ[(size_t)P.tile_J[P.u_tlo[P.fg_unit[P.fg_ptr[g]]]]].push_back((int32_t)P.n_cslots);
            ++P.n_cslots;
        }
        P.jslot_ptr.assign((size_t)nJ + 1, 0);
        for (int32_t J = 0; J < nJ; ++J) {
            std::sort(byJ[J].begin(), byJ[J].end());
            P.jslot.insert(P.jslot.end(), byJ[J].begin(), byJ[J].end());
            P.jslot_ptr[J + 1] = (int32_t)P.jslot.size();
        }
        if (P.n_cslots > INT32_MAX / kW) HH_THROW(HH_ERR_ARG, "plan too large (column slots)");
    }
    {
        // the tiled list by cost class (bit length of words + per-tile cost),
        // largest first, row order within a class: the remainder units of the
        // row-blocks form the launch's tail.  Dispatch order only: a row's
        // partials are summed in unit-index order (k_marg), bitwise the same.
        // (the flat list stays in row order: sorted too, C4 sweep +1 %,
        // profiles/r2b_modes_ab.log)
        std::vector<int64_t> key(P.u_tlo.size());
        for (size_t u = 0; u < key.size(); ++u) {
            int64_t c = (int64_t)(P.u_thi[u] - P.u_tlo[u]) * tile_fixed;
            for (int32_t t = P.u_tlo[u]; t < P.u_thi[u]; ++t) c += tile_words(t, P.u_rlo[u], P.u_rhi[u]);
            key[u] = 64 - __builtin_clzll((unsigned long long)c | 1ull);
        }
        const auto mid = P.u_order.end() - P.n_units_flat;
        auto by = [&](int32_t a, int32_t b) { return key[a] > key[b]; };
        std::stable_sort(P.u_order.begin(), mid, by);
    }
    if (P.n_part > INT32_MAX || P.tile_J.size() > (size_t)INT32_MAX) HH_THROW(HH_ERR_ARG, "plan too large");
    return P;
}

// One block per column-grouped flat tile, one wave per step chunk: the
// chunk's 64 U uint4 in registers (every load done before any store: in
// place), stored in the other order.  INV: interleaved -> plain.
template <bool INV>
__global__ __launch_bounds__(256) void k_flat_interleave(const FlatDesc* __restrict__ desc, uint16_t* __restrict__ payn) {
    constexpr int U = kFlatIlvU;
    const FlatDesc d = desc[blockIdx.x];
    uint4* __restrict__ p = reinterpret_cast<uint4*>(payn + d.entn);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (uint32_t q0 = 64u * U * (uint32_t)w; q0 < d.qbn; q0 += 64u * U * (uint32_t)nw) {
        const uint32_t m = d.qbn - q0 < 64u * U ? d.qbn - q0 : 64u * U;
        uint4 v[U];
        uint32_t src[U], dst[U];
        bool ok[U];
        uint32_t base = 0;
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const uint32_t plain = (uint32_t)lane * U + k, ilv = base + (uint32_t)lane;
            ok[k] = plain < m;
            src[k] = q0 + (INV ? ilv : plain);
            dst[k] = q0 + (INV ? plain : ilv);
            base += flat_ilv_cnt(m, k);
        }
#pragma unroll
        for (int k = 0; k < U; ++k) v[k] = p[ok[k] ? src[k] : q0];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the whole chunk read before it is rewritten
#pragma unroll
        for (int k = 0; k < U; ++k)
            if (ok[k]) p[dst[k]] = v[k];
    }
}

void finalize_flat_layout(hh_matrix& m, hipStream_t s) {
    m.flat_perm = 0;
    if (!m.n_fgroups || !m.fg_desc.n) return;
    hipLaunchKernelGGL(k_flat_interleave<false>, dim3((unsigned)m.fg_desc.n), dim3(256), 0, s, m.fg_desc.p, m.payn.p);
    HIP_CHECK(hipGetLastError());
    m.flat_perm = 1;
}

void narrow_payload_plain(const hh_matrix& m, DBuf<uint16_t>& out, hipStream_t s) {
    out.alloc(std::max<size_t>(m.payn.n, 1));
    if (m.payn.n) HIP_CHECK(hipMemcpyAsync(out.p, m.payn.p, m.payn.bytes(), hipMemcpyDeviceToDevice, s));
    if (m.flat_perm && m.fg_desc.n)
        hipLaunchKernelGGL(k_flat_interleave<true>, dim3((unsigned)m.fg_desc.n), dim3(256), 0, s, m.fg_desc.p, out.p);
    HIP_CHECK(hipGetLastError());
}

void upload_plan(const TilePlan& P, hh_matrix& m, hipStream_t s) {
    m.nJ = P.nJ;
    m.nrb = P.nrb;
    m.n_tiles = (int64_t)P.tile_J.size();
    m.n_units = (int64_t)P.u_tlo.size();
    m.n_units_flat = P.n_units_flat;
    m.payload_bytes_flat = P.payload_bytes_flat;
    m.n_part = P.n_part;
    m.n_slots = P.n_entries_padded;
    m.n_slots_narrow = P.n_narrow_padded;
    m.tile_J = to_device(P.tile_J, s);
    m.tile_rb = to_device(P.tile_rb, s);
    std::vector<long long> te(P.tile_ent.begin(), P.tile_ent.end());
    m.tile_ent = to_device(te, s);
    m.tile_rp = to_device(P.tile_rp, s);
    std::vector<long long> ten(P.tile_entn.begin(), P.tile_entn.end());
    m.tile_entn = to_device(ten, s);
    m.tile_rpn = to_device(P.tile_rpn, s);
    m.blk_tile_ptr = to_device(P.blk_tile_ptr, s);
    m.u_tlo = to_device(P.u_tlo, s);
    m.u_thi = to_device(P.u_thi, s);
    m.u_rb = to_device(P.u_rb, s);
    m.u_rlo = to_device(P.u_rlo, s);
    m.u_rhi = to_device(P.u_rhi, s);
    m.u_slot = to_device(P.u_slot, s);
    m.u_glo = to_device(P.u_glo, s);
    m.u_ghi = to_device(P.u_ghi, s);
    m.blk_unit_ptr = to_device(P.blk_unit_ptr, s);
    m.u_order = to_device(P.u_order, s);
    m.tile_perm = to_device(P.tile_perm, s);
    m.tile_band = to_device(P.tile_band, s);
    m.tile_fw = to_device(P.tile_fw, s);
    m.tile_frec = to_device(P.tile_frec, s);
    m.frec = to_device(P.frec, s);
    m.u_whole = to_device(P.u_whole, s);
    m.n_fgroups = P.fg_ptr.empty() ? 0 : (int64_t)P.fg_ptr.size() - 1;
    if (m.n_fgroups) {
        m.fg_ptr = to_device(P.fg_ptr, s);
        m.fg_unit = to_device(P.fg_unit, s);
        m.fg_desc = to_device(P.fg_desc, s);
    }
    m.upper = P.upper;
    m.n_cslots = P.n_cslots;
    if (P.upper) {
        m.u_cslot = to_device(P.u_cslot, s);
        if (!P.fg_cslot.empty()) m.fg_cslot = to_device(P.fg_cslot, s);
        m.jslot_ptr = to_device(P.jslot_ptr, s);
        if (!P.jslot.empty()) m.jslot = to_device(P.jslot, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));  // the plan's host vectors may die after return
}

}  // namespace hh

using namespace hh;

extern "C" {

const char* hh_last_error(void) { return g_last_error.c_str(); }
int hh_version(void) { return (0 << 16) | (2 << 8) | 0; }

int hh_ktime_enable(int32_t on) {
    return guard([&] { hh::g_ktime_on = on != 0; });
}

int hh_ktime_query(const char* name, double* total_ms, int64_t* calls) {
    return guard([&] {
        HH_REQUIRE(name && total_ms && calls, "bad arguments");
        std::lock_guard<std::mutex> lk(hh::g_ktime_mu);
        double t = 0.0;
        int64_t c = 0;
        for (auto& r : hh::g_ktime) {
            if (std::strcmp(r.name, name) != 0) continue;
            HIP_CHECK(hipEventSynchronize(r.b));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
            t += ms;
            ++c;
        }
        *total_ms = t;
        *calls = c;
    });
}

int hh_ktime_reset(void) {
    return guard([&] {
        std::lock_guard<std::mutex> lk(hh::g_ktime_mu);
        for (auto& r : hh::g_ktime) {
            (void)hipEventSynchronize(r.b);
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        hh::g_ktime.clear();
    });
}

int hh_device_count(int32_t* n) {
    return guard([&] {
        int c = 0;
        HIP_CHECK(hipGetDeviceCount(&c));
        *n = c;
    });
}

int hh_set_device(int32_t device) {
    return guard([&] { HIP_CHECK(hipSetDevice(device)); });
}

int hh_synchronize(void* stream) {
    return guard([&] { HIP_CHECK(hipStreamSynchronize(as_stream(stream))); });
}

int hh_device_copy(void* dst, const void* src, int64_t bytes, void* stream) {
    return guard([&] {
        HH_REQUIRE(bytes >= 0 && (bytes == 0 || (dst && src)), "bad arguments");
        if (bytes) HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    });
}

int hh_matrix_from_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                          int64_t n_bins, const int64_t* chrom_offsets, int32_t n_chroms,
                          int32_t ignore_diags, int32_t cis_only, int64_t row_lo, int64_t row_hi,
                          void* stream, hh_matrix** out) {
    return guard([&] {
        // cooler's sorted upper-triangle table: built on the device (build.hip);
        // any other order (or g_host_build): the host builder below
        if (!g_host_build &&
            build_from_host_pixels_on_device(bin1, bin2, count, nnz, n_bins, chrom_offsets, n_chroms, ignore_diags,
                                             cis_only, row_lo, row_hi, as_stream(stream), out))
            return;
        HH_REQUIRE(out && n_bins > 0 && nnz >= 0 && n_chroms > 0 && chrom_offsets, "bad arguments");
        HH_REQUIRE(nnz == 0 || (bin1 && bin2 && count), "null pixel arrays");
        HH_REQUIRE(n_bins < kMaxBins, "n_bins must be < 2^30");
        HH_REQUIRE(0 <= row_lo && row_lo <= row_hi && row_hi <= n_bins, "bad row range");
        HH_REQUIRE((row_lo % kR == 0 || row_lo == n_bins) && (row_hi % kR == 0 || row_hi == n_bins),
                   "shard rows must be aligned to 512-row blocks");
        HH_REQUIRE(chrom_offsets[0] == 0 && chrom_offsets[n_chroms] == n_bins, "chrom_offsets must span [0, n_bins]");
        HH_REQUIRE(n_chroms < 65535, "too many chromosomes");
        HH_REQUIRE(ignore_diags >= 0, "ignore_diags must be >= 0");
        hipStream_t s = as_stream(stream);
        auto m = std::make_unique<hh_matrix>();
        HIP_CHECK(hipGetDevice(&m->device));
        m->n_bins = n_bins;
        m->row_lo = row_lo;
        m->row_hi = row_hi;
        m->n_chroms = n_chroms;
        m->ignore_diags = ignore_diags;
        m->cis_only = cis_only ? 1 : 0;
        m->chrom_offsets.assign(chrom_offsets, chrom_offsets + n_chroms + 1);
        std::vector<int32_t> chrom_of(n_bins);
        for (int c = 0; c < n_chroms; ++c) {
            HH_REQUIRE(chrom_offsets[c] <= chrom_offsets[c + 1], "chrom_offsets not monotone");
            for (int64_t b = chrom_offsets[c]; b < chrom_offsets[c + 1]; ++b) chrom_of[b] = c;
        }
        const int64_t nloc = row_hi - row_lo;
        std::vector<double> diag(nloc, 0.0), rnnz(nloc, 0.0), rsum(nloc, 0.0);
        std::vector<int64_t> deg(nloc + 1, 0);
        auto keep = [&](int64_t i, int64_t& a, int64_t& b, uint32_t& c) -> bool {
            a = bin1[i];
            b = bin2[i];
            const double v = count[i];
            if (a > b) std::swap(a, b);
            if (a < 0 || b >= n_bins) HH_THROW(HH_ERR_ARG, "bin id out of range at pixel " + std::to_string(i));
            if (!(v >= 0.0) || v != std::floor(v) || v >= 4294967296.0)
                HH_THROW(HH_ERR_ARG, "counts must be non-negative integers < 2^32 (pixel " + std::to_string(i) + ")");
            if (v == 0.0) return false;
            if (cis_only && chrom_of[a] != chrom_of[b]) return false;
            if (b - a < ignore_diags) return false;
            c = (uint32_t)v;
            return true;
        };
        // pass 1: validate, filter, count row degrees, marginals
        int64_t nnz_upper = 0;
        for (int64_t i = 0; i < nnz; ++i) {
            int64_t a, b;
            uint32_t c;
            if (!keep(i, a, b, c)) continue;
            const bool ina = a >= row_lo && a < row_hi, inb = b >= row_lo && b < row_hi;
            if (a == b) {
                if (ina) {
                    if (diag[a - row_lo] != 0.0)
                        HH_THROW(HH_ERR_ARG, "duplicate pixel (" + std::to_string(a) + ", " + std::to_string(b) +
                                                 "): cooler's pixel table has unique (bin1, bin2)");
                    diag[a - row_lo] += c;
                    rnnz[a - row_lo] += 2.0;
                    rsum[a - row_lo] += 2.0 * c;
                    ++nnz_upper;
                }
                continue;
            }
            if (ina) { ++deg[a - row_lo + 1]; ++nnz_upper; rnnz[a - row_lo] += 1.0; rsum[a - row_lo] += c; }
            if (inb) { ++deg[b - row_lo + 1]; rnnz[b - row_lo] += 1.0; rsum[b - row_lo] += c; }
        }
        for (int64_t r = 0; r < nloc; ++r) deg[r + 1] += deg[r];
        // dense band width from the diagonals' occupancy over the WHOLE matrix
        // (identical for every shard: the band decomposition fixes the
        // summation order, so it must not depend on the row range)
        int32_t W = 0, W4 = 0;
        {
            std::vector<double> occ(kBandMaxW + 2, 0.0), big(kBandMaxW + 2, 0.0);
            for (int64_t i = 0; i < nnz; ++i) {
                int64_t a, b;
                uint32_t c;
                if (!keep(i, a, b, c) || a == b || b - a > kBandMaxW + 1) continue;
                occ[b - a] += 1.0;
                if (c > kBand4MaxCnt) big[b - a] += 1.0;
            }
            for (int64_t d = 1; d < (int64_t)occ.size(); ++d) {
                big[d] = occ[d] > 0 ? big[d] / occ[d] : 0.0;
                occ[d] = d < n_bins ? occ[d] / (double)(n_bins - d) : 0.0;
            }
            const BandWidths bw = choose_band_widths(occ, big, ignore_diags);
            W = bw.w8;
            W4 = bw.w4;
        }
        // (g_band_cis: trans pixels stay out of both bands)
        m->band_cis = g_band_cis ? 1 : 0;
        auto cis_ok = [&](int64_t r_glob, int64_t col) { return !m->band_cis || chrom_of[r_glob] == chrom_of[col]; };
        auto in_band = [&](int64_t r_glob, int64_t col, uint32_t v) {
            const int64_t d = col - r_glob;
            return W > 0 && v <= kBandMaxCnt && d != 0 && d >= -W && d <= W && cis_ok(r_glob, col);
        };
        auto in_nib = [&](int64_t r_glob, int64_t col, uint32_t v) {
            return in_band4(col - r_glob, v, W, W4) && cis_ok(r_glob, col);
        };
        // pass 2: symmetric CSR rows
        std::vector<int32_t> cols(deg[nloc]);
        std::vector<uint32_t> vals(deg[nloc]);
        {
            std::vector<int64_t> pos(deg.begin(), deg.end() - 1);
            for (int64_t i = 0; i < nnz; ++i) {
                int64_t a, b;
                uint32_t c;
                if (!keep(i, a, b, c) || a == b) continue;
                if (a >= row_lo && a < row_hi) { cols[pos[a - row_lo]] = (int32_t)b; vals[pos[a - row_lo]++] = c; }
                if (b >= row_lo && b < row_hi) { cols[pos[b - row_lo]] = (int32_t)a; vals[pos[b - row_lo]++] = c; }
            }
        }
        std::vector<std::pair<int32_t, uint32_t>> tmp;
        for (int64_t r = 0; r < nloc; ++r) {
            const int64_t lo = deg[r], hi = deg[r + 1];
            if (!std::is_sorted(cols.begin() + lo, cols.begin() + hi)) {
                tmp.clear();
                for (int64_t k = lo; k < hi; ++k) tmp.emplace_back(cols[k], vals[k]);
                std::stable_sort(tmp.begin(), tmp.end(), [](auto& x, auto& y) { return x.first < y.first; });
                for (int64_t k = lo; k < hi; ++k) { cols[k] = tmp[k - lo].first; vals[k] = tmp[k - lo].second; }
            }
            // a repeated (bin1, bin2) would be counted twice by the filters'
            // marginals but once by the dense bands: reject it (cooler's
            // pixel table is unique)
            for (int64_t k = lo + 1; k < hi; ++k)
                if (cols[k] == cols[k - 1])
                    HH_THROW(HH_ERR_ARG, "duplicate pixel (" + std::to_string(std::min<int64_t>(row_lo + r, cols[k])) +
                                             ", " + std::to_string(std::max<int64_t>(row_lo + r, cols[k])) +
                                             "): cooler's pixel table has unique (bin1, bin2)");
        }
        // tile counts: narrow (count <= 7) and wide entries per (row, tile);
        // counts > kCntMax go to the wide list
        const int32_t nJ = (int32_t)((n_bins + kW - 1) / kW);
        const bool upper = upper_tiles_on(nJ);
        std::vector<uint16_t> cntw((size_t)nloc * nJ, 0), cntn((size_t)nloc * nJ, 0);
        std::vector<long long> wptr(nloc + 1, 0);
        std::vector<uint8_t> band((size_t)nloc * band_stride(W), 0);
        std::vector<uint8_t> band4((size_t)nloc * band4_stride(W, W4), 0);
        int64_t n_band = 0;
        for (int64_t r = 0; r < nloc; ++r) {
            for (int64_t k = deg[r]; k < deg[r + 1]; ++k) {
                if (in_band(row_lo + r, cols[k], vals[k])) {
                    band[(size_t)r * band_stride(W) + band_slot(cols[k] - (row_lo + r), W)] = (uint8_t)vals[k];
                    ++n_band;
                    continue;
                }
                if (in_nib(row_lo + r, cols[k], vals[k])) {
                    const int64_t nib = band4_nibble(cols[k] - (row_lo + r), W, W4);
                    band4[(size_t)r * band4_stride(W, W4) + (nib >> 1)] |= (uint8_t)(vals[k] << (4 * (nib & 1)));
                    ++n_band;
                    continue;
                }
                if (vals[k] > kCntMax) ++wptr[r + 1];
                else if (upper && (cols[k] >> kWBits) < ((row_lo + r) >> kWBits)) continue;  // stored as its mirror
                else if (vals[k] <= kNarrowMax) ++cntn[(size_t)r * nJ + (cols[k] >> kWBits)];
                else ++cntw[(size_t)r * nJ + (cols[k] >> kWBits)];
            }
        }
        for (int64_t r = 0; r < nloc; ++r) wptr[r + 1] += wptr[r];
        std::vector<uint16_t> bg = bin_groups(*m);
        std::vector<uint16_t> rgroup(bg.begin() + row_lo, bg.begin() + row_hi);
        TilePlan P = plan_tiles(cntw.data(), cntn.data(), nloc, nJ, rgroup, row_lo, upper);
        // fill payloads + wide list
        std::vector<uint32_t> pay(P.n_entries_padded, 0u);
        std::vector<uint16_t> payn(P.n_narrow_padded, 0u);
        std::vector<int32_t> wcol(wptr[nloc]);
        std::vector<double> wcnt(wptr[nloc]);
        for (int64_t r = 0; r < nloc; ++r) {
            const int64_t rb = r / kR, k = r % kR;
            int32_t curJ = -1;
            int64_t pos = 0, posn = 0;
            int64_t wp = wptr[r];
            for (int64_t q = deg[r]; q < deg[r + 1]; ++q) {
                if (in_band(row_lo + r, cols[q], vals[q]) || in_nib(row_lo + r, cols[q], vals[q])) continue;
                if (vals[q] > kCntMax) { wcol[wp] = cols[q]; wcnt[wp++] = vals[q]; continue; }
                const int32_t J = cols[q] >> kWBits;
                if (upper && J < (int32_t)((row_lo + r) >> kWBits)) continue;
                if (J != curJ) {
                    const int32_t t = P.tile_of[rb * nJ + J];
                    pos = P.tile_ent[t] + P.tile_rp[(size_t)t * (kR + 1) + k];
                    posn = P.tile_entn[t] + P.tile_rpn[(size_t)t * (kR + 1) + k];
                    curJ = J;
                }
                if (vals[q] <= kNarrowMax) payn[posn++] = enc_narrow((uint32_t)cols[q] & kColMask, vals[q]);
                else pay[pos++] = enc_wide((uint32_t)cols[q] & kColMask, vals[q]);
            }
        }
        upload_plan(P, *m, s);
        m->pay = to_device(pay, s);
        m->payn = to_device(payn, s);
        m->wide_ptr = to_device(wptr, s);
        m->wide_col = to_device(wcol, s);
        m->wide_cnt = to_device(wcnt, s);
        m->n_wide = wptr[nloc];
        m->diag = to_device(diag, s);
        m->row_nnz2 = to_device(rnnz, s);
        m->row_sum2 = to_device(rsum, s);
        m->row_group = to_device(rgroup, s);
        m->band_w = W;
        m->band_w4 = W4;
        m->n_band = n_band;
        m->band = to_device(band, s);
        m->band4 = to_device(band4, s);
        m->nnz_upper = nnz_upper;
        m->n_entries = deg[nloc];
        finalize_flat_layout(*m, s);
        HIP_CHECK(hipStreamSynchronize(s));  // host vectors die here
        *out = m.release();
    });
}

int hh_matrix_free(hh_matrix* m) {
    return guard([&] {
        if (m) device_quiesce(m->device);
        delete m;
    });
}

int hh_matrix_get_info(const hh_matrix* m, hh_matrix_info* info) {
    return guard([&] {
        HH_REQUIRE(m && info, "null");
        info->n_bins = m->n_bins;
        info->row_lo = m->row_lo;
        info->row_hi = m->row_hi;
        info->nnz_upper = m->nnz_upper;
        info->n_entries = m->n_entries;
        info->n_slots = m->n_slots;
        info->n_tiles = m->n_tiles;
        info->n_units = m->n_units;
        info->n_wide = m->n_wide;
        info->device_bytes = (int64_t)m->device_bytes();
        info->n_slots_narrow = m->n_slots_narrow;
        info->payload_bytes = 4 * m->n_slots + 2 * m->n_slots_narrow + (int64_t)m->band.n + (int64_t)m->band4.n;
        info->band_w4 = m->band_w4;
        info->upper = m->upper;
        info->band_w = m->band_w;
        info->n_units_flat = (int32_t)m->n_units_flat;
        info->n_band = m->n_band;
        info->payload_bytes_flat = m->payload_bytes_flat;
        info->n_chroms = m->n_chroms;
        info->ignore_diags = m->ignore_diags;
        info->cis_only = m->cis_only;
        info->device = m->device;
    });
}

int hh_matrix_export_upper(const hh_matrix* m, int64_t* bin1, int64_t* bin2, double* count,
                           int64_t* nnz_inout) {
    return guard([&] {
        HH_REQUIRE(m && nnz_inout, "null");
        HIP_CHECK(hipSetDevice(m->device));
        const int64_t nloc = m->nloc();
        HIP_CHECK(hipDeviceSynchronize());
        std::vector<uint32_t> pay(m->pay.n), rp(m->tile_rp.n), rpn(m->tile_rpn.n);
        std::vector<uint16_t> payn(m->payn.n);
        std::vector<int32_t> tJ(m->tile_J.n), trb(m->tile_rb.n), wcol(m->wide_col.n);
        std::vector<long long> tent(m->tile_ent.n), tentn(m->tile_entn.n), wptr(m->wide_ptr.n);
        DBuf<uint16_t> plain;
        narrow_payload_plain(*m, plain, 0);
        plain.download(payn.data(), payn.size(), 0);
        m->tile_rpn.download(rpn.data(), rpn.size(), 0);
        m->tile_entn.download(tentn.data(), tentn.size(), 0);
        std::vector<double> wcnt(m->wide_cnt.n), diag(nloc);
        m->pay.download(pay.data(), pay.size(), 0);
        m->tile_rp.download(rp.data(), rp.size(), 0);
        m->tile_J.download(tJ.data(), tJ.size(), 0);
        m->tile_rb.download(trb.data(), trb.size(), 0);
        m->tile_ent.download(tent.data(), tent.size(), 0);
        m->wide_ptr.download(wptr.data(), wptr.size(), 0);
        m->wide_col.download(wcol.data(), wcol.size(), 0);
        m->wide_cnt.download(wcnt.data(), wcnt.size(), 0);
        m->diag.download(diag.data(), nloc, 0);
        HIP_CHECK(hipDeviceSynchronize());
        std::vector<std::vector<std::pair<int64_t, double>>> rows(nloc);
        for (size_t t = 0; t < tJ.size(); ++t) {
            const uint32_t* trp = &rp[t * (kR + 1)];
            const uint32_t* trpn = &rpn[t * (kR + 1)];
            for (int k = 0; k < kR; ++k) {
                const int64_t r = (int64_t)trb[t] * kR + k;
                for (uint32_t q = trp[k]; q < trp[k + 1]; ++q) {
                    const uint32_t e = pay[tent[t] + q];
                    const uint32_t c = e >> 16;
                    if (!c) continue;
                    rows[r].emplace_back((int64_t)tJ[t] * kW + dec_col(e), (double)c);
                }
                for (uint32_t q = trpn[k]; q < trpn[k + 1]; ++q) {
                    const uint32_t e = payn[tentn[t] + q];
                    const uint32_t c = e & 7u;
                    if (!c) continue;
                    rows[r].emplace_back((int64_t)tJ[t] * kW + dec_col(e), (double)c);
                }
            }
        }
        for (int64_t r = 0; r < nloc; ++r)
            for (long long q = wptr[r]; q < wptr[r + 1]; ++q) rows[r].emplace_back(wcol[q], wcnt[q]);
        if (m->band_w > 0) {
            const int64_t W = m->band_w;
            std::vector<uint8_t> band(m->band.n);
            m->band.download(band.data(), band.size(), 0);
            HIP_CHECK(hipDeviceSynchronize());
            for (int64_t r = 0; r < nloc; ++r)
                for (int64_t sl = 0; sl < band_stride(W); ++sl) {
                    const uint8_t v = band[(size_t)r * band_stride(W) + sl];
                    if (v) rows[r].emplace_back(m->row_lo + r + band_diag(sl, W), (double)v);
                }
        }
        if (m->band_w4 > m->band_w) {
            const int64_t W8 = m->band_w, W4 = m->band_w4, st = band4_stride(W8, W4);
            std::vector<uint8_t> b4(m->band4.n);
            m->band4.download(b4.data(), b4.size(), 0);
            HIP_CHECK(hipDeviceSynchronize());
            for (int64_t r = 0; r < nloc; ++r)
                for (int64_t d = -W4; d <= W4; ++d) {
                    if (d >= -W8 && d <= W8) continue;
                    const int64_t nib = band4_nibble(d, W8, W4);
                    const uint32_t v = (b4[(size_t)r * st + (nib >> 1)] >> (4 * (nib & 1))) & 15u;
                    if (v) rows[r].emplace_back(m->row_lo + r + d, (double)v);
                }
        }
        int64_t cnt = 0;
        const int64_t cap = *nnz_inout;
        auto emit = [&](int64_t i, int64_t j, double v) {
            if (v == 0.0) return;
            if (cnt < cap && bin1) { bin1[cnt] = i; bin2[cnt] = j; count[cnt] = v; }
            ++cnt;
        };
        for (int64_t r = 0; r < nloc; ++r) {
            const int64_t gr = m->row_lo + r;
            emit(gr, gr, diag[r]);
            std::sort(rows[r].begin(), rows[r].end());
            for (auto& e : rows[r])
                if (e.first > gr) emit(gr, e.first, e.second);
        }
        *nnz_inout = cnt;
    });
}

}  // extern "C"
