/*
 * hichap_hip.h — C-ABI of libhichap_hip.so, the MI355X (gfx950) hot path of
 * HiCHap's bias correction and structure analysis.
 *
 * Plain C types only (no torch / HIP types in signatures: streams are passed
 * as `void*` = hipStream_t, device buffers as plain pointers).  Every entry
 * point returns HH_OK (0) or a negative HH_ERR_* code; on error the message is
 * available from hh_last_error() (thread-local) and output buffers are left
 * untouched.  No C++ exception crosses this boundary.
 *
 * What each entry point replaces in the reference (/root/reference):
 *   ICE                 `cooler balance --ignore-diags 1 [--cis-only] --force`
 *                       subprocess strings, HiCHap/matrixBuilding.py:708, :713,
 *                       :1537, :1542, :1761, :1766 (algorithm: cooler.balance,
 *                       third-party, see oracle/ice_ref.py)
 *   hh_twostep          TwoStepCorrection, matrixBuilding.py:984-1023
 *   hh_genomewide_*     GenomeWideMatrixCorrection, matrixBuilding.py:857-901
 *   hh_compartment_*    StructureFind.Distance_Decay / Get_PCA / Select_PC_new,
 *                       StructureFind.py:201-423
 *   hh_di_scan          StructureFind.Get_Gap / Get_DI, StructureFind.py:721-839
 *   hh_insulation_*     nothing: the insulation score is defined by this project
 *                       (DESIGN.md §4k), fed from the same band as hh_di_scan
 *   hh_expected_pixels  nothing: defined by this project
 *   hh_saddle_pixels    nothing: defined by this project
 *   hh_pileup_pixels    nothing: defined by this project
 *   hh_domain_pileup_pixels  nothing: defined by this project
 *   hh_scc_pixels  nothing: defined by this project
 *   hh_trans_blocks / hh_trans_saddle  nothing: defined by this project
 *   hh_teig_*      nothing: defined by this project
 *   hh_symtab_*    nothing: defined by this project
 *   hh_viterbi_gmm      StructureFind.viterbipath (ghmm model.viterbi),
 *                       StructureFind.py:1113-1123 (host code)
 *   hh_hmm_bw_*         StructureFind.updateParameter / modelTrain (ghmm
 *                       model.baumWelch), StructureFind.py:1052-1110
 *   hh_hiccups_*      StructureFind.pcaller neighbourhood sums (HICCUPS loops),
 *                       StructureFind.py:1631-1830
 *   hh_binner_*         the per-line pair binning loops of TraditionalMatrixBuilding
 *                       (matrixBuilding.py:566-596), TraditionalMatrixInAllelic
 *                       (:817-854) and HaplotypeMatrixBuilding's unimputed
 *                       M_M / P_P / M_P / P_M passes (:1126-1240)
 */
#ifndef HICHAP_HIP_H
#define HICHAP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HH_OK 0
#define HH_ERR_ARG -1   /* invalid argument / unsupported input            */
#define HH_ERR_HIP -2   /* HIP runtime error                               */
#define HH_ERR_OOM -3   /* device or host allocation failed                */
#define HH_ERR_STATE -4 /* call not valid in the object's current state    */

/* ------------------------------------------------------------ runtime */
const char* hh_last_error(void);
int hh_version(void);                 /* (major<<16)|(minor<<8)|patch */
int hh_device_count(int32_t* n);
int hh_set_device(int32_t device);
int hh_synchronize(void* stream);
/* device-to-device copy of `bytes` on `stream` (asynchronous) */
int hh_device_copy(void* dst, const void* src, int64_t bytes, void* stream);
/* Tuning knobs, by name.  The table in hichap_master_amd/csrc/tune.hip is the
 * list: one row per key with its allowed values and what it does.  An unknown
 * key or a value outside the allowed ones returns HH_ERR_ARG, and
 * hh_last_error() then names the key and the allowed values; a value is never
 * replaced by another.
 * Results: "fuse_stats", "syrk_split", "pileup_chunk", "scc_rows" and
 * "trans_trips" change reduction orders (last bits), "band_cis" 0 regroups the sums of the rows whose trans
 * pixels lie inside the band widths (last bits), "parse_ablate" gives wrong
 * results while set; every other key leaves every bit unchanged.
 * When: the layout keys (band_w, band4, band_cis, flat_max, flat_cols,
 * flat_group, unit_entries, upper_tiles, host_build) act on matrices built
 * afterwards, "uband" on states created afterwards, the rest on the next call
 * that reads them.  "upper_tiles" 1 needs the 4096-column build. */
int hh_tune(const char* key, int64_t value);
/* The value in force for `key` (as hh_tune takes it). */
int hh_tune_get(const char* key, int64_t* value);
/* The last traced single-launch sweep: *n blocks; out (cap >= 3 n words) gets
 * (start, end, cu) per block in grid order (tiled units | band blocks | flat
 * units), wall-clock ticks (100 MHz).  Diagnostic, synchronising. */
int hh_sweep_trace(uint64_t* out, int64_t cap, int64_t* n);
/* Kernel timing (measurement only): while enabled, the dense-path launches
 * (k_rowstats, k_symvc1..3, k_syrk, k_cor_mul, k_select_stats, k_di,
 * k_gap_scan) are bracketed by HIP events on their stream; query returns the
 * summed duration and launch count for one kernel name (synchronising). */
int hh_ktime_enable(int32_t on);
int hh_ktime_query(const char* name, double* total_ms, int64_t* calls);
int hh_ktime_reset(void);

/* ---------------------------------------------------- contact matrix
 * A contact matrix resident in HBM in the "tiled pixel" layout:
 * the symmetric matrix (both triangles of cooler's upper-triangle pixel table)
 * for the rows [row_lo, row_hi) a rank owns, cut into 512-row blocks x
 * 8192-column tiles; each tile stores its rows' entries as uint16
 * (swizzled LDS byte offset << 3 | count, counts 1..7) and uint32 (count << 16 |
 * offset, counts 8..65535)
 * segments, rows padded to 16 B, counts > 65535 in a small per-row wide
 * list, plus a per-row diagonal.  Pixels near the diagonal (|col - row| <= W8,
 * count <= 255) live in a dense uint8 band with implicit columns, and those
 * with W8 < |col - row| <= W4 and count <= 15 in a dense 4-bit band, instead
 * of the tiles (W8, W4 chosen from the data's diagonal occupancy and counts).  Static filters
 * (ignore_diags, cis_only zero_trans, zero counts) are applied at build time.
 * Shards are whole 512-row blocks (row_lo % 512 == 0).
 */
typedef struct hh_matrix hh_matrix;

typedef struct {
    int64_t n_bins;        /* bins of the whole matrix                       */
    int64_t row_lo, row_hi;/* rows held by this object                      */
    int64_t nnz_upper;     /* kept pixels with bin2 - bin1 >= ignore_diags   */
    int64_t n_entries;     /* symmetric off-diagonal entries stored          */
    int64_t n_slots;       /* stored uint32 slots (entries + row padding)    */
    int64_t n_tiles;       /* nonempty (row-block, column-tile) pairs        */
    int64_t n_units;       /* sweep work units                               */
    int64_t n_wide;        /* entries with count >= 2^19 (wide list)         */
    int64_t device_bytes;  /* HBM held by the matrix                         */
    int64_t n_slots_narrow;/* stored uint16 slots (entries + row padding)    */
    int64_t payload_bytes; /* entry bytes streamed per sweep (both widths and
                              the dense band)                                */
    int32_t n_chroms;
    int32_t ignore_diags;
    int32_t cis_only;
    int32_t device;
    int32_t band_w;        /* uint8 diagonal band half-width W8 (0 = none)   */
    int32_t n_units_flat;  /* work units swept by the flat (short-row) kernel */
    int64_t n_band;        /* nonzero entries held by the band               */
    int64_t payload_bytes_flat; /* part of payload_bytes in flat-kernel tiles */
    int32_t band_w4;       /* nibble band outer width (== band_w: none)      */
    int32_t upper;         /* 1: upper-triangle tiles         */
} hh_matrix_info;

/* Build from cooler's pixel table (host arrays; any order: a sorted
 * upper-triangle table is uploaded and built on the device, anything else is
 * built on the host; duplicate (bin1, bin2) pixels fail with HH_ERR_ARG).  Counts must be non-negative integers < 2^32
 * (cooler `count`, int32 in HiCHap's traditional coolers, matrixBuilding.py:196).
 * chrom_offsets[n_chroms+1] = cooler `indexes/chrom_offset`. Rows outside
 * [row_lo, row_hi) are not stored (a shard for multi-GPU genome-wide ICE). */
int hh_matrix_from_pixels(const int64_t* bin1, const int64_t* bin2, const double* count,
                          int64_t nnz, int64_t n_bins, const int64_t* chrom_offsets,
                          int32_t n_chroms, int32_t ignore_diags, int32_t cis_only,
                          int64_t row_lo, int64_t row_hi, void* stream, hh_matrix** out);
/* The same from a DEVICE pixel table in cooler's own order — sorted by
 * (bin1, bin2), bin1 <= bin2, unique — with int32 ids and counts (cooler's
 * `count` dtype for HiCHap's traditional coolers; what hh_binner_pixels_device
 * hands out).  Built entirely on the device (filters, symmetric rows by a
 * radix sort of the lower half, tile counts, payload); the layout equals
 * hh_matrix_from_pixels'.  A table out of order, with a duplicate pixel, a
 * negative count or an id out of range fails with HH_ERR_ARG naming the first
 * offending pixel.  hh_matrix_from_pixels itself takes this path whenever its
 * host table is sorted upper-triangle (uploading it once), and builds on the
 * host otherwise (hh_tune "host_build" 1 forces the host builder). */
int hh_matrix_from_pixels_device(const int32_t* bin1, const int32_t* bin2, const int32_t* count, int64_t nnz,
                                 int64_t n_bins, const int64_t* chrom_offsets, int32_t n_chroms, int32_t ignore_diags,
                                 int32_t cis_only, int64_t row_lo, int64_t row_hi, void* stream, hh_matrix** out);
int hh_matrix_free(hh_matrix* m);
int hh_matrix_get_info(const hh_matrix* m, hh_matrix_info* info);
/* Diagnostic read rates of a matrix's own buffers (no sweep work): out[2i] =
 * ms per pass, out[2i+1] = bytes, for i = 0 wide / 1 narrow tile entries,
 * 2 uint8 / 3 nibble band (linear reads), 4-6 the flat tiles' payload in the
 * flat sweep's order, streamed only; 7-8 the same with coalesced run loads;
 * 9 the narrow entries linearly in lane-major runs.  nout >= 20. */
int hh_matrix_stream_probe(const hh_matrix* m, int32_t reps, double* out, int32_t nout);
/* Copy the stored upper-triangle pixels (bin1 <= bin2, bin1 in the local rows
 * for which bin1 is the row) back to the host; *nnz_inout = capacity on entry,
 * count on exit.  For checking only. */
int hh_matrix_export_upper(const hh_matrix* m, int64_t* bin1, int64_t* bin2, double* count,
                           int64_t* nnz_inout);

/* Synthetic whole-genome contact matrices generated directly in HBM
 * (SURVEY.md §8(d) model; counter-based hashing keyed on the unordered bin
 * pair, so every shard of every rank sees the same matrix). */
typedef struct {
    int32_t n_chroms;
    const int32_t* chrom_nbins; /* host array [n_chroms]                     */
    double A;                   /* cis amplitude                              */
    double decay;               /* power-law exponent (1.08)                  */
    double comp_strength;       /* 0.3                                        */
    double vis_sigma;           /* log-normal visibility sigma (0.3)          */
    double gap_frac;            /* fraction of empty bins (0.02)              */
    double trans_density;       /* uniform trans pixel density                */
    int32_t comp_block;         /* compartment block length in bins           */
    int32_t ignore_diags;
    int32_t cis_only;
    int32_t pad_;
    uint64_t seed;
} hh_synth_params;

/* Counting pass over ALL rows: per-row stored slots (work) and upper-triangle
 * pixel counts (host arrays of n_bins).  Used to partition rows across ranks. */
int hh_synth_count(const hh_synth_params* p, int32_t* row_work, int64_t* row_nnz_upper,
                   void* stream);
/* Dense cis block of chromosome `chrom` of the same synthetic genome as
 * float64 counts into device memory out[N_c * N_c] (bench inputs for the
 * per-chromosome compartment config C5; ignore_diags applies). */
int hh_synth_dense(const hh_synth_params* p, int32_t chrom, double* out, void* stream);
/* The model's pixel table in HBM (bench inputs of the table-driven paths):
 * cooler's upper-triangle table sorted by (bin1, bin2), or with ordered = 1
 * every nonzero cell (i, j) sorted by (i, j) with independent draws for (i, j)
 * and (j, i) (an asymmetric matrix like HiCHap's imputed haplotype matrices).
 * int32 ids and counts, owned by the hh_pixels handle. */
typedef struct hh_pixels hh_pixels;
int hh_synth_pixels(const hh_synth_params* p, int32_t ordered, void* stream, hh_pixels** out);
int hh_pixels_get(const hh_pixels* P, const int32_t** bin1, const int32_t** bin2, const int32_t** count, int64_t* nnz);
int hh_pixels_free(hh_pixels* P);
/* Build rows [row_lo, row_hi) (row_lo % 512 == 0). */
int hh_synth_build(const hh_synth_params* p, int64_t row_lo, int64_t row_hi, void* stream,
                   hh_matrix** out);

/* ---------------------------------------------------------------- ICE
 * cooler's balance_cooler semantics (oracle/ice_ref.py). */
typedef struct {
    int32_t mad_max;           /* 5                                         */
    int32_t min_nnz;           /* 10                                        */
    double min_count;          /* 0                                         */
    double tol;                /* 1e-5                                      */
    int32_t max_iters;         /* 200                                       */
    int32_t rescale_marginals; /* 1                                         */
    int32_t check_every;       /* host polls convergence every k sweeps (0=8)*/
    int32_t pad_;
} hh_ice_opts;

/* One-call balance on one GPU (the matrix must hold every row).
 * weights[n_bins] (host) receive cooler's bins/weight (NaN = masked).
 * Per group (1 group genome-wide, n_chroms groups when cis_only):
 * scale[], var[], iters[], converged[] (host arrays).
 * sweep_seconds (may be NULL) = wall time of the iteration loop only. */
int hh_ice_balance(hh_matrix* m, const hh_ice_opts* o, double* weights, double* scale,
                   double* var, int32_t* iters, int32_t* converged, double* sweep_seconds,
                   void* stream);

/* Fine-grained device API used by the multi-GPU driver (one process per GPU;
 * the marginal vector is exchanged with an all-gather over RCCL by the
 * caller).  All calls are asynchronous on `stream` unless noted. */
typedef struct hh_ice hh_ice;
int hh_ice_create(hh_matrix* m, const hh_ice_opts* o, hh_ice** out);
int hh_ice_free(hh_ice* s);
int hh_ice_n_groups(const hh_ice* s, int32_t* n);
/* mode: 0 = binarized (nnz), 1 = raw counts, 2 = count*b_i*b_j.
 * Writes the marginal of the local rows to marg_local[row_hi - row_lo]
 * (device).  When the matrix holds every row, marg_local may be NULL and the
 * result lands in the internal full marginal directly. */
int hh_ice_marg_local(hh_ice* s, int32_t mode, double* marg_local, void* stream);
/* Scatter an all-gathered, per-rank padded marginal (world x maxlen, device)
 * into the internal full marginal; rank_rows[world+1] host row offsets. */
int hh_ice_set_marg(hh_ice* s, const double* gathered, int32_t world, int64_t maxlen,
                    const int64_t* rank_rows, void* stream);
/* Filters (after set_marg of the matching mode).  mad uses host medians:
 * synchronous. */
int hh_ice_filter_nnz(hh_ice* s, void* stream);
int hh_ice_filter_count_mad(hh_ice* s, void* stream);
/* One ICE update after set_marg(mode 2): variance, bias update, convergence. */
int hh_ice_update(hh_ice* s, void* stream);
/* Number of still-active groups (synchronous). */
int hh_ice_active_groups(hh_ice* s, int32_t* n_active, void* stream);
int hh_ice_iterations_done(const hh_ice* s, int32_t* iters);
/* Full sweeps on one GPU without host polling (bench / single-GPU): runs
 * `n` iterations of marg(mode 2) + update back to back. */
int hh_ice_run(hh_ice* s, int32_t n, void* stream);
/* Final weights + stats (synchronous), as hh_ice_balance. */
int hh_ice_finalize(hh_ice* s, double* weights, double* scale, double* var, int32_t* iters,
                    int32_t* converged, void* stream);
/* Kernel timing of the last hh_ice_run (HIP events on the run's stream):
 * total ms of the sweep kernel, launches. */
int hh_ice_last_sweep_timing(const hh_ice* s, double* sweep_ms_total, int32_t* sweep_launches,
                             double* iter_ms_total);
/* The schedule this state's next weighted sweep takes under the current
 * hh_tune settings (hh_tune "sweep_sched"): 0 = one stream; 1 = all
 * concurrent, the flat, tiled and band kernels started together on up to
 * three streams; 2 = phased, the flat kernel alone, then the tiled kernel and
 * the band sweep side by side; 3 = the whole sweep in one launch.  Host only,
 * no synchronisation. */
int hh_ice_sweep_sched(const hh_ice* s, int32_t* sched);
/* Payload bytes one sweep of this state reads: tile entries + both segments'
 * row pointers + the band bytes its band kernels stream (the upper halves
 * only, plus a shard's halo rows, with the upper-band sweep).
 * A measurement helper (bench.py's roofline), no computation. */
int hh_ice_swept_bytes(const hh_ice* s, int64_t* bytes);
/* The current bias vector b (all n_bins entries, every rank holds the whole
 * vector; 0 = masked) to host memory (synchronous; checking only: the
 * marginal of the next sweep is marg_i = b_i sum_j A_ij b_j). */
int hh_ice_get_bias(const hh_ice* s, double* bias, void* stream);
/* The mirror: replace the bias vector by bias[n_bins] (host; synchronous;
 * checking only: chosen biases in front of one hh_ice_marg_local(2)).  Not
 * with upper-triangle tiles, whose fixed-point scale follows the updates. */
int hh_ice_set_bias(hh_ice* s, const double* bias, void* stream);
/* Upper-band sweep (hh_tune "ub_fast", default 1: counts enter the FMAs as
 * exponent-zero doubles, biases staged times 2^512; 0: converted counts
 * everywhere; the same bits either way): the workgroups since hh_ice_create
 * whose staged biases were not all 0 or of magnitude in [2^-400, 2^400] and
 * which therefore took the conversion walk (0 without the upper-band sweep;
 * synchronous). */
int hh_ice_uband_fallbacks(const hh_ice* s, int64_t* count, void* stream);
/* Upper-band sweep, dead rectangles (hh_tune "ub_skip", default 1): with the
 * cis-only band layout (hh_tune "band_cis", default 1) a wave task (128 rows
 * x one 1008-slot chunk) whose slots all lie past its rows' chromosome ends
 * holds only zeros and is not walked.  *all_waves: the wave tasks of this
 * shard's workgroups with a row below n_bins; *dead_waves: the dead ones among
 * them (0 for a matrix built with band_cis 0, and without the upper-band
 * sweep).  From the chromosome offsets alone: host, no synchronisation,
 * independent of "ub_skip". */
int hh_ice_uband_skipped(const hh_ice* s, int64_t* dead_waves, int64_t* all_waves);

/* ------------------------------------------------ sharded ICE in C
 * Genome-wide ICE over world processes (one GPU each), each holding the
 * matrix rows rank_rows[rank] .. rank_rows[rank + 1] (whole 512-row blocks):
 * per iteration one all-gather of the local marginals, then the identical
 * update everywhere, iterations enqueued from C++ (no caller code in the
 * loop).  The exchange is a callback: `allgather(send, count, recv, user,
 * stream)` must gather `count` doubles from every rank (device buffers,
 * rank order) into recv[world * count] on `stream` and return 0.  The
 * library's RCCL transport: hh_comm_unique_id on one rank (128 bytes, shared
 * by the caller's own means), hh_comm_init on every rank, then pass
 * hh_comm_allgather with user = the hh_comm. */
typedef int (*hh_allgather_fn)(const double* send, int64_t count, double* recv, void* user, void* stream);
typedef struct hh_comm hh_comm;
int hh_comm_unique_id(uint8_t* id128);
int hh_comm_init(const uint8_t* id128, int32_t world, int32_t rank, hh_comm** out);
int hh_comm_free(hh_comm* c);
int hh_comm_allgather(const double* send, int64_t count, double* recv, void* comm, void* stream);
/* Upper-triangle tiles store an entry of a strictly upper
 * tile once, and its column side belongs to the rank owning that column: a
 * shard's marginals need a second exchange per sweep, an int64 reduce-scatter
 * of the ranks' padded row blocks (integer sums: exact, the same bits on any
 * number of ranks).  `reduce(send, count, recv, user, stream)`: send = world x
 * count int64 (rank-major blocks), recv = count: the sum over the ranks of this
 * rank's block; 0 = ok.  hh_comm_reduce_scatter is RCCL's (user = the
 * hh_comm).  hh_ice_*_sharded register the exchange themselves (RCCL's when
 * their all-gather is hh_comm_allgather, else a reduction through the
 * all-gather callback: world x its bytes); a caller that drives
 * hh_ice_marg_local on a shard registers it once after hh_ice_create
 * (rank -1: inferred from the matrix's row range; reduce NULL keeps one
 * registered before for the same world). */
typedef int (*hh_reduce_fn)(const int64_t* send, int64_t count, int64_t* recv, void* user, void* stream);
int hh_comm_reduce_scatter(const int64_t* send, int64_t count, int64_t* recv, void* comm, void* stream);
int hh_ice_set_column_exchange(hh_ice* s, int32_t world, int32_t rank, const int64_t* rank_rows, hh_reduce_fn reduce,
                               void* reduce_user, hh_allgather_fn allgather, void* allgather_user);
/* The whole balance (filters, iterations to convergence, finalize) on this
 * rank's shard `m`; outputs as hh_ice_balance (weights for every bin, identical
 * on every rank). */
int hh_ice_balance_sharded(hh_matrix* m, const hh_ice_opts* o, int32_t world, int32_t rank, const int64_t* rank_rows,
                           hh_allgather_fn allgather, void* user, double* weights, double* scale, double* var,
                           int32_t* iters, int32_t* converged, double* sweep_seconds, void* stream);
/* `cooler balance --cis-only` (matrixBuilding.py:713, :1542, :1766) over world
 * processes with no collective in the iterations:
 * every rank holds whole chromosomes (dealt by LPT on their pixels) as a
 * compact cis-only matrix `m` -- its chromosomes' bins renumbered
 * consecutively -- whose per-chromosome ICE groups converge independently.
 * The one exchange is `allgather` of max_local_bins doubles per rank (the
 * per-chromosome-normalised raw marginals, zero padded) for cooler's
 * genome-wide MAD cutoff.  Outputs cover this rank's bins and chromosomes. */
int hh_ice_balance_cis_local(hh_matrix* m, const hh_ice_opts* o, int32_t world, int64_t max_local_bins,
                             hh_allgather_fn allgather, void* user, double* weights, double* scale, double* var,
                             int32_t* iters, int32_t* converged, double* sweep_seconds, void* stream);
/* Pieces of it on an hh_ice (bench / fixed iteration counts): the two
 * filters, and n iterations without convergence polling. */
int hh_ice_filters_sharded(hh_ice* s, int32_t world, const int64_t* rank_rows, hh_allgather_fn allgather, void* user,
                           void* stream);
int hh_ice_run_sharded(hh_ice* s, int32_t world, const int64_t* rank_rows, hh_allgather_fn allgather, void* user,
                       int32_t n, void* stream);

/* ------------------------------------------ dense two-step correction
 * Dense row-major N x N matrices; dtype 0 = int64, 1 = float64.  Host
 * pointers (copied in/out) or, with on_device = 1, device pointers. */
/* Per row i over columns [lo[i], hi[i]) (lo = hi = NULL: whole rows): sum
 * (exact for int64) and number of zero entries.  Replaces the row loops of
 * Coverage_M / Gap_defined / Gap_definedLowRes and the alpha row sums,
 * matrixBuilding.py:742-753, :878-881, :904-929, :994-995. */
int hh_dense_rowstats(const void* X, int32_t dtype, int64_t N, const int64_t* lo, const int64_t* hi,
                      double* rowsum, int64_t* zeros, int32_t on_device, void* stream);
/* out = (raw_sum / N^2) / mean(C) * C with C = Correct_VC(Y, exponent),
 * Y = Trans2symmetry(X / alpha[:, None], gap) (gap = NULL: the sum form,
 * Trans2symmetryLowRes).  raw_sum = sum(X) (MM.mean() * N^2).
 * TwoStepCorrection :1007-1021, GenomeWideMatrixCorrection :894-899. */
int hh_dense_symvc(const void* X, int32_t dtype, int64_t N, const double* alpha, const uint8_t* gap,
                   double exponent, double raw_sum, double* out, int32_t on_device, void* stream);
/* TwoStepCorrection(TM, MM, PM) (matrixBuilding.py:984-1023) in one call:
 * int64 N x N inputs, float64 N x N outputs (Nor_MM, Nor_PM), gap masks
 * (gap_m[i] = 1 for i in Gap_M).  The gap / alpha glue runs on the host with
 * np.percentile ('linear') semantics; each matrix crosses PCIe once. */
/* Dense N x N int64 (device `out`, zeroed first) from cells (row, col, count)
 * whose ids are shifted by `offset`: out[r][c] = count, and out[c][r] too for
 * an upper-triangle table (symmetric = 1).  The reference's dense matrices
 * from its per-line loops (matrixBuilding.py:554, :567-570, :1290-1301), built
 * on the device from the binner's tables so only the cells cross PCIe.
 * Cells must be unique; out-of-range ids (or bin1 > bin2 when symmetric)
 * are an error.  on_device = 1: row / col / count are device pointers. */
int hh_dense_from_cells(const int64_t* row, const int64_t* col, const int64_t* count, int64_t nnz, int64_t N,
                        int64_t offset, int32_t symmetric, int32_t on_device, int64_t* out, void* stream);
/* Upper-triangle nonzeros of a dense fp64 N x N device matrix in cooler
 * order, the np.triu(M).nonzero() table NPZ2Cooler writes for the corrected
 * matrices (matrixBuilding.py:1613, :1628-1633): hh_dense_upper_count, then
 * hh_dense_upper_write into caller-sized device buffers. */
int hh_dense_upper_count(const double* X, int64_t N, int64_t* nnz, void* stream);
int hh_dense_upper_write(const double* X, int64_t N, int32_t* bin1, int32_t* bin2, double* value, void* stream);
int hh_twostep(const int64_t* TM, const int64_t* MM, const int64_t* PM, int64_t N, double* nor_mm, double* nor_pm,
               uint8_t* gap_m, uint8_t* gap_p, int32_t on_device, void* stream);
/* IntraChromMatrixCorrection (matrixBuilding.py:1026-1041): hh_twostep over
 * n chromosomes in one call, device pointers only (TM[c], MM[c], PM[c] int64
 * N[c] x N[c]; nor_mm[c], nor_pm[c] fp64 outputs).  The row statistics and
 * the gap / alpha glue of every chromosome run as shared launches; then
 * n_streams = 0: every pass of every chromosome's two symmetrisation chains
 * in one shared launch per pass; 1..16: each chain's launches on the
 * least-loaded of that many streams, largest chromosomes first.  One
 * synchronisation at the end; per chromosome bitwise hh_twostep's results.
 * gap_m / gap_p (host) receive every chromosome's flags concatenated in
 * argument order. */
int hh_twostep_batch(int32_t n, const int64_t* const* TM, const int64_t* const* MM, const int64_t* const* PM,
                     const int64_t* N, double* const* nor_mm, double* const* nor_pm, uint8_t* gap_m,
                     uint8_t* gap_p, int32_t n_streams, void* stream);

/* ------------------------------------ sparse genome-wide correction
 * GenomeWideMatrixCorrection (matrixBuilding.py:857-901) on pixel tables
 * instead of dense 2n x 2n matrices.  T: the traditional whole-genome table
 * (cooler order: bin1 <= bin2, sorted, unique) on n bins, chrom_offsets[n_chroms
 * + 1] its chromosome layout; H: every nonzero cell (row, col, count) of the
 * imputed haplotype matrix, sorted by (row, col), unique, on 2n bins laid out
 * as the M copies of the chromosomes then the P copies (Get_Chro_Bins_Haplotypes
 * :429-454).  hh_gw_create validates both and computes the alpha step's exact
 * integer statistics; the caller computes alpha (NumPy percentile semantics,
 * :878-893) and hh_gw_correct does S = H / Alpha[:, None], the sum
 * symmetrisation (:770-777), Correct_VC(., exponent) and the mean rescale
 * (:894-899), leaving the upper triangle of the result (cooler order, what
 * NPZ2Cooler stores) on the device.  Counts are integers < 2^32. */
typedef struct hh_gw hh_gw;
int hh_gw_create(const int64_t* t_bin1, const int64_t* t_bin2, const double* t_count, int64_t t_nnz,
                 const int64_t* h_row, const int64_t* h_col, const double* h_count, int64_t h_nnz, int64_t n,
                 const int64_t* chrom_offsets, int32_t n_chroms, void* stream, hh_gw** out);
/* the same from device int32 tables (the binner's outputs) */
int hh_gw_create_device(const int32_t* t_bin1, const int32_t* t_bin2, const int32_t* t_count, int64_t t_nnz,
                        const int32_t* h_row, const int32_t* h_col, const int32_t* h_count, int64_t h_nnz, int64_t n,
                        const int64_t* chrom_offsets, int32_t n_chroms, void* stream, hh_gw** out);
int hh_gw_free(hh_gw* g);
/* host arrays: t_rowsum[n], t_nnz_row[n] = sum / nonzero count of T's row
 * within its chromosome block (the diagonal once); h_blocksum[2n] = sum of H's
 * row within its same-chromosome same-haplotype block (M_M / P_P); *h_total =
 * sum(H).  Any pointer may be NULL. */
int hh_gw_stats(const hh_gw* g, int64_t* t_rowsum, int64_t* t_nnz_row, int64_t* h_blocksum, int64_t* h_total);
/* The alpha step (:878-893) per chromosome on those statistics, computed by
 * hh_gw_create on a host thread while the column lists build: alpha[n] in
 * bin order, chrom_ok[n_chroms] (layout order) 0 where the caller must use
 * NumPy's own path (no non-gap bin, or a max that is not positive finite).
 * Replaces matrixBuilding.py:878-886's Python loop. */
int hh_gw_alpha(const hh_gw* g, double* alpha, int32_t* chrom_ok);
/* alpha[2n] (host): the concatenated, duplicated SNP-density factors;
 * exponent: 2/3.  *out_nnz = upper-triangle pixels of the result. */
int hh_gw_correct(hh_gw* g, const double* alpha, double exponent, int64_t* out_nnz, void* stream);
/* hh_gw_correct in two calls, the output owned by the caller: the count
 * (marginals, VC factors, merge count pass, the mean rescale factor; state
 * kept in the handle), then the write of the upper table into device
 * buffers of out_nnz elements. */
int hh_gw_correct_count(hh_gw* g, const double* alpha, double exponent, int64_t* out_nnz, void* stream);
int hh_gw_correct_write(hh_gw* g, int32_t* bin1, int32_t* bin2, double* value, void* stream);
/* the result to host arrays of out_nnz (any may be NULL), or its device
 * pointers (valid until hh_gw_free or the next hh_gw_correct) */
int hh_gw_result(const hh_gw* g, int64_t* bin1, int64_t* bin2, double* value, void* stream);
int hh_gw_result_device(const hh_gw* g, const int32_t** bin1, const int32_t** bin2, const double** value);

/* ---------------------------------------------------- compartment (one chrom)
 * StructureFind.Distance_Decay / Get_PCA / Select_PC_new, StructureFind.py:201-423.
 * M: dense N x N float64 raw contacts (cooler matrix(balance=False).fetch). */
typedef struct hh_comp hh_comp;
int hh_comp_create(const double* M, int64_t N, int32_t on_device, void* stream, hh_comp** out);
int hh_comp_free(hh_comp* c);
/* nnz_col[j] = number of nonzero entries of column j (gap columns, :216-220). */
int hh_comp_colnnz(hh_comp* c, int64_t* nnz_col, void* stream);
/* sums[d] = sum of nonzero M[i][j] with |i-j| = d whose column j is not a gap
 * (gapcol[j] = 1) — the bincount of Distance_Decay before the bin_num division. */
int hh_comp_diag_sums(hh_comp* c, const uint8_t* gapcol, double* sums, void* stream);
/* Get_PCA(SA=True): the Sliding_Approach O/E (StructureFind.py:274-299,
 * step = 600000 // Res // 2 >= 1) materialised on the device (N x N): box
 * sum of M over the (2 step + 1)^2 window / the 3-2-1 weighted expected sum
 * inside [step, N - step - 1]^2, M / decline[|i-j|] on the border.  Later
 * hh_comp_correlation / hh_comp_select_stats use it in place of the plain
 * O/E; decline = NULL switches back. */
int hh_comp_sliding_oe(hh_comp* c, const double* decline, int32_t step, void* stream);
int hh_comp_get_sliding_oe(hh_comp* c, double* oe, void* stream);
/* O/E = M / decline[|i-j|] on nonzeros (or the Sliding_Approach O/E), columns
 * ng[0..n); Pearson correlation of those columns (np.corrcoef(rowvar=False),
 * NaN -> 0; the diagonal of a column with nonzero variance exactly 1) kept on
 * the device. */
int hh_comp_correlation(hh_comp* c, const double* decline, const int64_t* ng, int64_t n, void* stream);
int hh_comp_get_cor(hh_comp* c, double* cor, void* stream);
/* Replace the device correlation (n x n from the last hh_comp_correlation). */
int hh_comp_set_cor(hh_comp* c, const double* cor, void* stream);
/* Top-k right singular vectors of the column-centred correlation (sklearn
 * PCA(k).fit(Cor).components_, sign: max-|.| entry positive), k x n row-major.
 * Default method (hh_tune "pca_method" 1): explicit-restart block Krylov on
 * Cor (16 columns, hh_tune "pca_p" products per cycle) with a Rayleigh-Ritz
 * step for the centred matrix; stops when the top-k Ritz vectors'
 * a-posteriori angle bound max ||A x - theta x|| / gap is < tol, or has
 * stopped shrinking below 1e3 tol (the rounding floor; a degenerate gap never
 * gets there), after at most 2 * max_iters Cor products.  Method 0
 * (and the fallback when the Krylov basis and its residual block would not
 * fit, n < 16 (pca_p + 1), or when Krylov's start block is rank deficient):
 * block subspace iteration with 16 columns, max_iters iterations.  n <= 16
 * (method 3, whatever "pca_method" says): the centred matrix has rank < 16,
 * so a 16-column block is singular there; the n x n correlation is downloaded
 * and the eigenvectors of Xc^T Xc come from a Jacobi iteration on the host,
 * always converged, no Cor products.  n < k is an error whose text gives n
 * (the reference's PCA raises there too).  *iters = Cor products (Krylov),
 * iterations (subspace) or 0 (host).  Not converging is not an error: query
 * hh_comp_pca_status.  The Krylov products read only the upper triangle of
 * Cor (hh_tune "cor_sym", default 1; 0: the full matrix), so a Cor set with
 * hh_comp_set_cor is taken as symmetric; hh_tune "ortho_tpb" / "ortho_min_tpb"
 * set the orthogonalisation's rows per block (/ 64). */
int hh_comp_pca(hh_comp* c, int32_t k, double tol, int32_t max_iters, double* components, double* eigvals,
                int32_t* iters, void* stream);
/* Outcome of the last hh_comp_pca: converged (1/0), Cor products, Krylov
 * cycles (subspace: iterations), method (1 Krylov, 2 Krylov redone without
 * k_ortho after its grid barrier timed out, 0 subspace, 3 host). */
int hh_comp_pca_status(const hh_comp* c, int32_t* converged, int32_t* products, int32_t* cycles, int32_t* method);
/* Host helper (no GPU): top-k eigenpairs, descending, of a symmetric m x m
 * matrix (Householder tridiagonalisation, implicit QL eigenvalues, inverse
 * iteration) — the Rayleigh-Ritz solver of the Krylov PCA; evecs m x k
 * row-major. */
int hh_sym_topk(const double* H, int32_t m, int32_t k, double* evals, double* evecs);
/* Per PC q < k (<= 3), 8 sums: [0,1] Cor same-sign pairs in (-1, 1-eps) sum,count;
 * [2,3] Cor (pc_i > 0, pc_j < 0) pairs in (-1, 1) sum,count; [4,5] nonzero O/E
 * over (+,+) sum,count; [6,7] over (-,-) — Select_PC_new's means_minus / select_ab. */
int hh_comp_select_stats(hh_comp* c, const double* pcs, int32_t k, double eps, double* stats, void* stream);

/* ------------------------------------------------------- TAD scan (DI)
 * Both scans read column j only within B rows of the diagonal, so the matrix
 * is passed as a diagonal-major band: band[(B + k) * N + j] = M[j + k][j],
 * k in [-B, B] (0 outside the matrix); M balanced with NaN -> 0 for traditional data.
 * hh_gap_scan = StructureFind.Get_Gap (:721-751): gap[j] = 1 when column j
 * has fewer than 2*lb*0.8 nonzeros in M[j-lb:j+lb, j] or is within lb of an
 * edge (lb <= B).  hh_di_scan = Get_DI (:804-839): di[j] from the up / down
 * windows of window_bins[j] <= B bins (0 at gap[j] and edges); test 0 =
 * t-test, 1 = chi-square. */
int hh_gap_scan(const double* band, int64_t N, int32_t B, int32_t lb, uint8_t* gap, int32_t on_device,
                void* stream);
int hh_di_scan(const double* band, int64_t N, int32_t B, const uint8_t* gap, const int32_t* window_bins,
               int32_t test, double* di, int32_t on_device, void* stream);
/* The same scans fed from cooler's pixel table instead of a dense matrix:
 * StructureFind.Data_preprocess (:853-854) loads each chromosome as
 * cooler.matrix(balance=True).fetch(chrom) + np.nan_to_num (allelic data:
 * balance=False, :858-865) and scans it.  hh_band_from_pixels builds that
 * matrix's band on the device, band[(B + k) * N + j] = M[j + k][j] for the
 * chromosome's bins [lo, lo + N), from the unique upper-triangle pixels
 * (bin1 <= bin2, global bin ids): value count * weight[bin1] * weight[bin2]
 * with NaN -> 0, or the raw count when weight is NULL (n_weight >= lo + N).
 * on_device: bin1/bin2/count/weight/band are device pointers; otherwise host
 * pointers (the band is returned to the host).  hh_tad_scan_pixels = band of
 * width B = max(lb, max window_bins) + hh_gap_scan + the first / last bin
 * joining the gap (Data_preprocess :876-884) + hh_di_scan in one call, the
 * pixel table crossing PCIe once (not at all with on_device); gap, di and
 * window_bins are host arrays of N. */
int hh_band_from_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                        const double* weight, int64_t n_weight, int64_t lo, int64_t N, int32_t B, double* band,
                        int32_t on_device, void* stream);
int hh_tad_scan_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                       const double* weight, int64_t n_weight, int64_t lo, int64_t N, int32_t lb,
                       const int32_t* window_bins, int32_t test, uint8_t* gap, double* di, int32_t on_device,
                       void* stream);

/* -------------------------------------------------- insulation score
 * Diamond sums of the insulation score (HiCHap has none: the
 * definition is this project's).  For bin i, window w and ignore_diags g the
 * diamond is C_w(i) = {(a, b): i - w < a <= i <= b < i + w, 0 <= a, b < N,
 * b - a >= g}; S[k * N + i] is the fp64 sum of M[a][b] over the cells of
 * C_windows[k](i) with valid[a] and valid[b], n[k * N + i] their number.
 * windows: 1..8 host values, each 1..256 bins, strictly ascending; one launch
 * serves them all, a window adding its shell to the next smaller one's sum.
 * Fixed summation order, no atomics: two calls give the same bits.
 * hh_insulation_scan reads the band of the DI scans (B >= 2 * max window - 2)
 * and valid (uint8[N], NULL = all valid).  hh_insulation_pixels builds the
 * band from cooler's pixel table as hh_band_from_pixels does (weight NULL =
 * raw counts) and scans it in one call, the pixel table crossing PCIe once;
 * valid[a] = 0 where weight is given and weight[lo + a] is not finite or
 * bad[a] != 0 (bad: uint8[N] or NULL).  nnz = 0 is valid (S = 0).
 * on_device: band / valid / bin1 / bin2 / count / weight / bad / S / n are
 * device pointers; otherwise host pointers.  HH_ERR_ARG (outputs untouched):
 * n_windows outside 1..8, a window outside 1..256, windows not ascending,
 * ignore_diags < 0, a band narrower than 2 * max window - 2, weights that do
 * not cover the chromosome. */
int hh_insulation_scan(const double* band, int64_t N, int32_t B, const uint8_t* valid, const int32_t* windows,
                       int32_t n_windows, int32_t ignore_diags, double* S, int32_t* n, int32_t on_device,
                       void* stream);
int hh_insulation_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                         const double* weight, int64_t n_weight, int64_t lo, int64_t N, const uint8_t* bad,
                         const int32_t* windows, int32_t n_windows, int32_t ignore_diags, double* S, int32_t* n,
                         int32_t on_device, void* stream);

/* ------------------------------------------------- TAD HMM (host code)
 * Viterbi path of a continuous HMM with Gaussian-mixture emissions, ghmm's
 * `model.viterbi(EmissionSequence)` as StructureFind.viterbipath calls it
 * (:1113-1123): S states, M components per state; A (S x S, row-major) and pi
 * are probabilities, mean / var / weight are S x M (var = variance, ghmm's
 * GaussianMixtureDistribution parameters).  Log space, a_ij = 0 -> -inf, ties
 * to the lowest state.  path[t] = state of obs[t]; *logp = log joint
 * probability of the path.  Runs on the host (no GPU needed). */
int hh_viterbi_gmm(const double* obs, int64_t n, int32_t S, int32_t M, const double* A, const double* pi,
                   const double* mean, const double* var, const double* weight, int32_t* path, double* logp);

/* ------------------------------------------------- TAD HMM training (GPU)
 * Baum-Welch re-estimation of the same model over K sequences, ghmm's
 * `model.baumWelch(SequenceSet)` as StructureFind.updateParameter calls it
 * (:1052-1088).  ghmm is absent: the algorithm is the one DESIGN.md §4f
 * defines (scaled forward / backward, emissions in log space with a
 * per-observation shift, batch M-step, variances floored at var_floor; a
 * re-estimate whose denominator is 0 keeps its old value, a_ij = 0 and
 * w_im = 0 stay 0), in fp64, bitwise reproducible.  1 <= S, M <= 8.
 *
 * hh_hmm_bw_create uploads the concatenated observations once; sequence q is
 * obs[seq_off[q] .. seq_off[q + 1]) (seq_off: n_seq + 1 entries from 0).  A
 * non-finite observation or an empty sequence fails with HH_ERR_ARG.
 * hh_hmm_bw_step runs one EM iteration: the host arrays A (S x S), pi (S),
 * mean / var / weight (S x M) are replaced by their re-estimates and *logp is
 * the log likelihood of all sequences under the parameters passed IN.  A
 * sequence no state path can emit fails with HH_ERR_ARG (parameters left
 * untouched).  hh_hmm_bw_train repeats it: iteration k (from 0) stores
 * logp_trace[k] = L_k, the log likelihood under the parameters entering it,
 * applies its M-step, and ends the run when k >= 1 and
 * 0 <= L_k - L_{k-1} < eps * |L_k|, or when k + 1 == max_iter.  *iters = the
 * iterations run (entries of logp_trace, which holds max_iter); *status = a
 * bit set of HH_BW_*.  hh_hmm_bw_last_step_ms: device time of the last
 * iteration's kernels (HIP events). */
typedef struct hh_hmm_bw hh_hmm_bw;
#define HH_BW_MAX_ITER 1     /* stopped by max_iter, not by the likelihood test   */
#define HH_BW_LOGP_DROPPED 2 /* some L_k < L_{k-1} - 1e-9 |L_k| (more than rounding) */
#define HH_BW_VAR_FLOORED 4  /* some re-estimated variance was raised to var_floor */
int hh_hmm_bw_create(const double* obs, const int64_t* seq_off, int64_t n_seq, int32_t S, int32_t M, void* stream,
                     hh_hmm_bw** out);
int hh_hmm_bw_free(hh_hmm_bw* h);
int hh_hmm_bw_step(hh_hmm_bw* h, double* A, double* pi, double* mean, double* var, double* weight,
                   double var_floor, double* logp);
int hh_hmm_bw_train(hh_hmm_bw* h, double* A, double* pi, double* mean, double* var, double* weight,
                    int32_t max_iter, double eps, double var_floor, int32_t* iters, double* logp_trace,
                    int32_t* status);
int hh_hmm_bw_last_step_ms(hh_hmm_bw* h, double* ms);

/* ---------------------------------------------------------- pair binning
 * Pair text (HiCHap *_Valid.bed: chrom/pos in fields 1, 6, 8, 13; allelic
 * beds: fields 0-3 and a trailing mark) -> cooler pixel tables per target
 * matrix: upper triangle (bin1 <= bin2), sorted by (bin1, bin2), count = number
 * of pairs of the unordered bin pair — what the reference's dense
 * `M[b1][b2] += 1; M[b2][b1] += 1` (once when b1 == b2) + np.triu + nonzero
 * produce (matrixBuilding.py:457-525, :566-596).
 * Lines follow Python's `line.strip().split()`; chromosome fields are
 * `lstrip('chr')`-ed and looked up in the name table.  A line the reference
 * would raise on (missing field, non-integer position, a name that passes the
 * `chroms` filter but is not in genomeSize, a bin outside the matrix) fails the
 * feed with HH_ERR_ARG naming the first such line (negative positions too:
 * the reference's NumPy indexing would wrap them). */
typedef struct hh_binner hh_binner;
typedef struct {
    int32_t col_chrom1, col_pos1, col_chrom2, col_pos2; /* 0-based fields      */
    char mark[16];     /* non-empty: skip lines whose LAST field differs (`if
                          line[-1] != 'Both': continue`, :1133)              */
    int32_t hap1, hap2;/* haplotype half of chrom1 / chrom2 (0 = M or the
                          traditional genome, 1 = P)                         */
    int32_t mode;      /* 0 binning; 1 imputation (HaplotypeMatrixBuilding
                          :1251-1494): lines whose last field == mark are
                          skipped, last field == mark2 selects the R1 branch  */
    char mark2[16];
} hh_pairs_format;
/* names: n_names NUL-terminated names back to back (after lstrip('chr'));
 * name_ids[k] = chromosome index (Sort_Chromosomes order) or -2 for a name
 * the `chroms` filter accepts but genomeSize lacks.  unknown_policy for names
 * not in the table: 0 skip the line, 1 raise if the name is all digits
 * ('#' in chroms), 2 raise (empty chroms list). */
int hh_binner_create(int32_t n_chroms, const char* names, const int32_t* name_ids, int32_t n_names,
                     int32_t unknown_policy, hh_binner** out);
int hh_binner_free(hh_binner* b);
/* One output matrix at resolution `res`: chrom_start[2 * n_chroms] = first
 * global bin of chromosome c in haplotype h (index h * n_chroms + c; the
 * traditional layout uses h = 0 only), chrom_nbins[c] = l // res + 1.
 * local = 1: intra-chromosome matrices only (localRes; trans pairs dropped,
 * per-chromosome bounds), bins still global (split per chromosome by the
 * caller). */
int hh_binner_add_target(hh_binner* b, int32_t res, int32_t local, const int64_t* chrom_start,
                         const int32_t* chrom_nbins, int64_t n_bins, int32_t* index_out);
/* An imputation target (ordered cells: the imputed matrices are asymmetric).
 * Whole (local = 0): `unimputed` = the unimputed whole matrix (host, n_bins x
 * n_bins int64, haplotype layout), L = Imputation_region // res, the
 * Imputation_min / _ratio tests.  Feeds in mode 1: first the M_M text
 * (hap 0), then — after hh_binner_set_stale — the P_P text (hap 1). */
int hh_binner_add_impute_target(hh_binner* b, int32_t res, int32_t local, const int64_t* chrom_start,
                                const int32_t* chrom_nbins, int64_t n_bins, const int64_t* unimputed, int32_t L,
                                int64_t imin, double ratio, int32_t* index_out);
/* The M pass's last line (byte offset in the concatenated feeds) that reached
 * the neighbourhood step, and at which target (-1 / -1: none): the caller
 * rebuilds the reference's stale M_M_sub from it and sets the P pass's sum
 * per whole target (ok = 0: the reference raises there). */
int hh_binner_last_reached(const hh_binner* b, int64_t* byte_offset, int32_t* target);
int hh_binner_set_stale(hh_binner* b, int32_t target, int64_t pp_sum, int32_t ok);
/* Parse + bin host text (staged through pinned chunks of chunk_bytes, cut at
 * line ends; 0 = 256 MB) or device-resident text.  Synchronous. */
int hh_binner_feed(hh_binner* b, const char* text, int64_t nbytes, const hh_pairs_format* f, int64_t chunk_bytes,
                   void* stream);
int hh_binner_feed_device(hh_binner* b, const char* text, int64_t nbytes, const hh_pairs_format* f, void* stream);
/* stats4: lines read, lines binned, skipped by the chromosome filter,
 * skipped by the mark filter. */
int hh_binner_stats(const hh_binner* b, int64_t* stats4);
/* Sort + run-length encode every target (synchronous); then nnz per target. */
int hh_binner_finish(hh_binner* b, void* stream);
int hh_binner_target_nnz(const hh_binner* b, int32_t target, int64_t* nnz, int64_t* n_pairs);
int hh_binner_download(const hh_binner* b, int32_t target, int32_t* bin1, int32_t* bin2, int32_t* count);
/* Device pointers of a finished target (valid until hh_binner_free). */
int hh_binner_pixels_device(const hh_binner* b, int32_t target, const int32_t** bin1, const int32_t** bin2,
                            const int32_t** count);
/* Synthetic pair text generated in device memory (bench input): format 0 =
 * 15-column *_Valid.bed lines, 1 = allelic "chrom pos chrom pos mark".  out =
 * NULL: size query into *nbytes. */
int hh_synth_pairs_text(int32_t n_chroms, const char* names, const int64_t* lengths, int64_t n_lines,
                        double cis_frac, double max_dist, int32_t format, uint64_t seed, int64_t line0, char* out,
                        int64_t capacity, int64_t* nbytes, void* stream);

/* ------------------------------------------------ HICCUPS loop calling
 * The neighbourhood sums of StructureFind.pcaller (StructureFind.py:1631-1830)
 * for one chromosome.  Bands are row-major N x num (num = maxapart / res +
 * maxww + 1; band[r][d] = M[r][r + d], 0 past the matrix): Hb raw counts with
 * the main diagonal zeroed, Cb balanced counts on diagonals ww..num-1 (0
 * elsewhere); Eall[d] = expected on diagonal d (0 for d < ww). */
typedef struct hh_hiccups hh_hiccups;
int hh_hiccups_create(const double* Hb, const double* Cb, const double* Eall, int64_t N, int32_t num, int32_t pw,
                      int32_t on_device, void* stream, hh_hiccups** out);
int hh_hiccups_free(hh_hiccups* h);
/* Candidate pixels (row <= col, col - row < num); resets every pixel to pending. */
int hh_hiccups_set_pixels(hh_hiccups* h, const int32_t* row, const int32_t* col, int64_t n, void* stream);
/* Every pixel back to pending (same pixels; repeated runs). */
int hh_hiccups_reset(hh_hiccups* h, void* stream);
/* One window width w (>= pw): every pending pixel whose lower-left raw reads
 * reach 16 gets its donut / lower-left balanced and expected sums and is
 * assigned; *newly_valid = how many (the caller applies the reference's
 * stop rule: fewer than 10 % of the pending pixels). */
int hh_hiccups_width(hh_hiccups* h, int32_t w, int64_t* newly_valid, void* stream);
/* Per pixel: donut / lower-left sums of the balanced (sK, sY) and expected
 * (eK, eY) bands at its width; width[i] = that w (0 = never assigned). */
int hh_hiccups_results(hh_hiccups* h, double* sK, double* sY, double* eK, double* eY, uint8_t* width, void* stream);

/* ------------------------------------------------ loop selection (rank)
 * StructureFind.Loop_Selecting (:2063-2094) keeps a called pixel by the rank
 * of its raw count within its own diagonal of the dense raw matrix:
 * bisect_left(sorted(M.diagonal(d)), M[r][c]).  hh_diag_rank_pixels computes
 * that from cooler's pixel table, one call per chromosome: bin1 <= bin2 are
 * global bin ids of unique pixels, the chromosome is bins [lo, lo + N);
 * pixels with either end outside it are ignored.  Queries are chromosome-
 * local, 0 <= qrow <= qcol < N, in any order, repeats allowed.  value[q] =
 * the raw count at (qrow, qcol), 0 when no pixel is stored there; less[q] =
 * how many of the N - d entries of diagonal d = qcol - qrow of the symmetric
 * dense matrix are < value[q] (0 when value[q] is 0).  Exact integers, the
 * same on every run.  A negative count or bin1 > bin2 on a pixel inside the
 * chromosome, and a query outside the range, fail with HH_ERR_ARG.  nnz = 0
 * and nq = 0 are valid.  on_device: bin1 / bin2 / count are device pointers;
 * the query and result arrays are host arrays either way.  Buckets in LDS
 * or in global memory: hh_tune("rank_lds_buckets"). */
int hh_diag_rank_pixels(const int64_t* bin1, const int64_t* bin2, const int64_t* count, int64_t nnz, int64_t lo,
                        int64_t N, const int32_t* qrow, const int32_t* qcol, int64_t nq, int64_t* value,
                        int64_t* less, int32_t on_device, void* stream);

/* ------------------------------------------------ allelic specificity
 * The reads of HiCHap/AllelicSpecificity.py from the dense raw matrix of one
 * chromosome (one cell per loop, :96-97; a 2 * offset square per boundary,
 * :297-302), gathered from cooler's pixel table: bin1 <= bin2 are global bin
 * ids of unique pixels SORTED by (bin1, bin2) (cooler's invariant), float64
 * counts, the chromosome is bins [lo, lo + N); pixels with either end outside
 * it are ignored.  Window k is the h x w block whose top-left cell is
 * chromosome-local (wrow[k], wcol[k]); out[(k * h + r) * w + c] = the count
 * stored at (min(i, j), max(i, j)), i = wrow[k] + r, j = wcol[k] + c, or 0.0
 * where no pixel is stored (the symmetric matrix; windows may lie on, above
 * or below the diagonal, overlap and repeat).  Exact copies, one writer per
 * cell.  A window leaving [0, N), bin1 > bin2 or a non-finite count on a
 * pixel inside the chromosome, and a table that is not strictly ascending in
 * (bin1, bin2) fail with HH_ERR_ARG.  nnz = 0 and nw = 0 are valid.
 * on_device: bin1 / bin2 / count / out are device pointers; wrow / wcol are
 * host arrays either way. */
int hh_pixel_windows(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz, int64_t lo,
                     int64_t N, const int32_t* wrow, const int32_t* wcol, int64_t nw, int32_t h, int32_t w,
                     double* out, int32_t on_device, void* stream);
/* less[k] = #{(i, j) : fl(a[i] - b[j]) < q[k]}, the plain fp64 subtract:
 * bisect_left(sorted(a_i - b_j for all i, j), q[k]) without the na * nb list
 * (CompartmentAllelicSpecificity.BackGround / Calculating, :460-485, :509).
 * Exact int64, the same on every run.  na, nb, nq < 2^31; non-finite inputs
 * fail with HH_ERR_ARG; empty a, b or q are valid.  on_device: a / b / q /
 * less are device pointers (the O(K) inputs are staged through the host for
 * the checks and the sort of b). */
int hh_pairdiff_rank(const double* a, int64_t na, const double* b, int64_t nb, const double* q, int64_t nq,
                     int64_t* less, int32_t on_device, void* stream);

/* ------------------------------------------------ coarsen (cooler coarsen / zoomify)
 * cooler's `coarsen` on cooler's own pixel table: fine bin i of chromosome c
 * maps to coarse bin coff_c + (i - off_c) / factor, coff the running sum of
 * ceil(nbins_c / factor) (a coarse bin never spans two chromosomes; the last
 * one of a chromosome may hold fewer fine bins).  Input: unique pixels sorted
 * by (bin1, bin2), bin1 <= bin2, integer counts >= 0, chrom_offsets[n_chroms
 * + 1] (host).  Output: again cooler's table (sorted, upper triangle, unique),
 * every count the exact integer sum of the fine pixels of its cell -- a cell
 * exists where a fine pixel maps to it, a stored 0 included; fine pixels (i,
 * j), i < j, of one coarse bin land on the coarse diagonal.  No key sort:
 * work items of (coarse row x HH_COARSEN_TILE coarse columns) sum in int64
 * LDS cells and write in item order, so the result is bitwise the same on
 * every run.  Two passes: hh_coarsen_count checks the table
 * and returns the number of coarse pixels and the largest coarse count, the
 * caller sizes the outputs (int32 counts hold while max_count <= 2^31 - 1,
 * int64 otherwise: nothing fails on overflow), hh_coarsen_write fills them,
 * hh_coarsen_free releases the handle.  A table that is out of order or has
 * a duplicate pixel, bin1 > bin2, an id outside [0, n_bins) or a negative
 * count fails the count pass with HH_ERR_ARG naming the first offending
 * pixel, as hh_matrix_from_pixels_device does; no handle is made.  nnz = 0 is
 * valid.  The sums must fit int64.
 * Device form: int32 ids, int32 or int64 (count_is_i64) counts -- on_device
 * = 1 device pointers (as hh_pixels_get / hh_binner_pixels_device hand them
 * out; they must stay valid and unchanged until hh_coarsen_write returns), 0
 * host arrays, uploaded; the outputs of hh_coarsen_write are device arrays of
 * out_nnz entries (int32 ids; counts int32, or int64 with count_is_i64).
 * Host form: int64 ids and counts as cooler stores them, host outputs (int64
 * ids).  The handle belongs to the device current at the count call; write
 * and free run there and restore the caller's device.  The tile width can be
 * lowered for the next count call with hh_tune("coarsen_tile", 64 ..
 * HH_COARSEN_TILE); hh_coarsen_tile reads the value in force. */
#define HH_COARSEN_TILE 8192
typedef struct hh_coarsen hh_coarsen;
int hh_coarsen_tile(int32_t* tile);
int hh_coarsen_count(const int32_t* bin1, const int32_t* bin2, const void* count, int32_t count_is_i64, int64_t nnz,
                     int64_t n_bins, const int64_t* chrom_offsets, int32_t n_chroms, int64_t factor,
                     int32_t on_device, void* stream, hh_coarsen** out, int64_t* out_nnz, int64_t* max_count);
int hh_coarsen_count_host(const int64_t* bin1, const int64_t* bin2, const int64_t* count, int64_t nnz, int64_t n_bins,
                          const int64_t* chrom_offsets, int32_t n_chroms, int64_t factor, void* stream,
                          hh_coarsen** out, int64_t* out_nnz, int64_t* max_count);
int hh_coarsen_write(const hh_coarsen* h, int32_t* out_bin1, int32_t* out_bin2, void* out_count,
                     int32_t count_is_i64, void* stream);
int hh_coarsen_write_host(const hh_coarsen* h, int64_t* out_bin1, int64_t* out_bin2, void* out_count,
                          int32_t count_is_i64, void* stream);
int hh_coarsen_free(hh_coarsen* h);

/* ------------------------------------------------ merge (cooler merge)
 *   hh_merge_*   cooler's `merge` on pixel tables
 * The union of n_tables (1 .. 64) pixel tables over the SAME bin table of
 * n_bins bins: the output holds every pixel present in at least one input,
 * its count the exact integer sum over the inputs -- a pixel exists where an
 * input stores it, a stored 0 included.  Every input is cooler's table: unique
 * pixels sorted by (bin1, bin2), bin1 <= bin2, integer counts >= 0; so is the
 * output.  It is hh_coarsen with factor 1 over several tables: work items of
 * (row x column tile) walk the tables' row segments as one range, sum in
 * int64 LDS cells and write in item order; no key sort, the same bits on
 * every run and for every order of the tables.  The column tile is the value
 * of hh_tune("coarsen_tile") at the count call.  One table is the identity.
 * Two passes as hh_coarsen: hh_merge_count checks every table and returns the
 * number of merged pixels and the largest merged count, the caller sizes the
 * outputs (int32 counts hold while max_count <= 2^31 - 1, int64 otherwise:
 * nothing fails on overflow), hh_merge_write fills them, hh_merge_free
 * releases the handle.  A table that is out of order or has a duplicate
 * pixel, bin1 > bin2, an id outside [0, n_bins) or a negative count fails the
 * count pass with HH_ERR_ARG "table <t>: <what> at pixel <i>", t the first
 * such table and i its first offending pixel; no handle is made.  Tables of
 * nnz = 0 (NULL arrays allowed) are valid.  The sums must fit int64.  The
 * handle holds 8 B per (table, row, column tile) until hh_merge_free: memory
 * bounds a call (HH_ERR_OOM, no handle) long before the argument limits do.
 * bin1 / bin2 / count are host arrays of n_tables pointers, nnz and
 * count_is_i64 host arrays of n_tables entries.
 * Device form: int32 ids, int32 or int64 (count_is_i64[t]) counts per table --
 * on_device = 1 device pointers (they must stay valid and unchanged until
 * hh_merge_write returns), 0 host arrays, uploaded; the outputs of
 * hh_merge_write are device arrays of out_nnz entries (int32 ids; counts
 * int32, or int64 with count_is_i64).  Host form: int64 ids and counts as
 * cooler stores them, host outputs (int64 ids).  The handle belongs to the
 * device current at the count call; write and free run there and restore the
 * caller's device. */
typedef struct hh_merge hh_merge;
int hh_merge_count(const int32_t* const* bin1, const int32_t* const* bin2, const void* const* count,
                   const int32_t* count_is_i64, const int64_t* nnz, int32_t n_tables, int64_t n_bins,
                   int32_t on_device, void* stream, hh_merge** out, int64_t* out_nnz, int64_t* max_count);
int hh_merge_count_host(const int64_t* const* bin1, const int64_t* const* bin2, const int64_t* const* count,
                        const int64_t* nnz, int32_t n_tables, int64_t n_bins, void* stream, hh_merge** out,
                        int64_t* out_nnz, int64_t* max_count);
int hh_merge_write(const hh_merge* h, int32_t* out_bin1, int32_t* out_bin2, void* out_count, int32_t count_is_i64,
                   void* stream);
int hh_merge_write_host(const hh_merge* h, int64_t* out_bin1, int64_t* out_bin2, void* out_count,
                        int32_t count_is_i64, void* stream);
int hh_merge_free(hh_merge* h);

/* ------------------------------------------------ down-sampling
 *   hh_sample_*   nothing: defined by this project
 * Binomial thinning of a pixel table by a counter-based rule.  With mix64 the
 * splitmix64 finaliser (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) *
 * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31),
 * for pixel (bin1, bin2) of count c
 *     base = mix64(seed ^ mix64(((uint64)bin1 << 32) | (uint64)bin2))
 *     kept = #{ t in [0, c) : mix64(base + t) < thr }     (uint64, wrapping)
 * the output holds the pixels with kept > 0, in the input's order, with kept
 * as their count.  thr = floor(frac 2^64) keeps each contact with probability
 * frac < 1 (thr = 0 keeps none; frac = 1 has no threshold: do not call).  A
 * contact's fate depends on (seed, bin1, bin2, t) alone: the result is the
 * same bits on every run, for host and device input, for a part of the table
 * as for the whole, and samples of one seed are nested (thr_a <= thr_b gives
 * kept_a <= kept_b for every pixel).  The cost is one mix64 per contact.
 * The input need not be sorted or unique; ids must lie in [0, 2^31) and counts
 * be >= 0, else the count pass fails with HH_ERR_ARG naming the first
 * offending pixel and no handle is made.  nnz = 0 is valid.
 * Two passes: hh_sample_count computes and stores every pixel's kept and
 * returns the number of kept pixels, the kept total and the largest kept
 * count; the caller sizes the outputs (counts int32, or int64 when max_count >
 * 2^31 - 1); hh_sample_write compacts; hh_sample_free releases the handle.
 * Forms, pointer lifetimes and device ownership as hh_merge / hh_coarsen. */
typedef struct hh_sample hh_sample;
int hh_sample_count(const int32_t* bin1, const int32_t* bin2, const void* count, int32_t count_is_i64, int64_t nnz,
                    uint64_t thr, uint64_t seed, int32_t on_device, void* stream, hh_sample** out, int64_t* out_nnz,
                    int64_t* kept_total, int64_t* max_count);
int hh_sample_count_host(const int64_t* bin1, const int64_t* bin2, const int64_t* count, int64_t nnz, uint64_t thr,
                         uint64_t seed, void* stream, hh_sample** out, int64_t* out_nnz, int64_t* kept_total,
                         int64_t* max_count);
int hh_sample_write(const hh_sample* h, int32_t* out_bin1, int32_t* out_bin2, void* out_count, int32_t count_is_i64,
                    void* stream);
int hh_sample_write_host(const hh_sample* h, int64_t* out_bin1, int64_t* out_bin2, void* out_count,
                         int32_t count_is_i64, void* stream);
int hh_sample_free(hh_sample* h);

/* ------------------------------------ cis expected and compartment saddle
 *   hh_expected_pixels / hh_saddle_pixels   nothing: defined by this project
 *                                           
 * Both read cooler's pixel table of one chromosome, global bins [lo, lo + N),
 * with hh_insulation_pixels' conventions: unique pixels sorted by (bin1,
 * bin2), bin1 <= bin2; a pixel with an end outside the chromosome is ignored;
 * the value of a cell is v(a, b) = count * weight[bin1] * weight[bin2] in that
 * order, NaN -> 0 (weight NULL: the raw count; n_weight >= lo + N otherwise);
 * valid[a] = 0 where weight is given and weight[lo + a] is not finite or
 * bad[a] != 0 (bad: uint8[N] or NULL).  nnz = 0 is valid.  No N x N matrix is
 * made: the table is streamed once per call.
 * hh_expected_pixels, for g = ignore_diags and D = max_dist: for g <= d <= D
 * sum[d] is the fp64 sum of v(a, a + d) over the stored pixels with valid[a]
 * and valid[a + d], nvalid[d] = #{a in [0, N - d): valid[a] and valid[a + d]}
 * (every cell, stored or not); both are 0 for d < g.  sum, nvalid: D + 1
 * entries.  The expected value of a diagonal is sum / nvalid (host).
 * hh_saddle_pixels: cls is uint8[N], class ids 0 .. K - 1 or 255 for a bin
 * left out; expected is double[D + 1]; a diagonal d in [min_dist, D] is usable
 * when expected[d] is finite and > 0.  For every cell a < b on a usable
 * diagonal with both bins valid and both classes != 255, Cu[cls[a] * K +
 * cls[b]] counts the cell and, where the cell is a stored pixel, U[cls[a] * K
 * + cls[b]] adds v(a, b) / expected[b - a] (an IEEE division).  U, Cu: K x K,
 * row-major; the symmetric saddle sums are U + U^T and Cu + Cu^T (host).
 * The fp64 sums have a fixed order and use no floating-point atomics: two
 * calls, the host and the device form and every hh_tune("saddle_diag_tile")
 * give the same bits; nvalid and Cu are exact integers.  Every index derived
 * from the table is range-checked before it addresses anything: a malformed
 * table may give wrong numbers, never an out-of-range access.
 * on_device: bin1 / bin2 / count / weight / bad / expected / cls and the
 * outputs are device pointers; otherwise host pointers.  HH_ERR_ARG (outputs
 * untouched): N < 1, max_dist outside [0, N - 1], ignore_diags < 0, min_dist
 * < 1 or > max_dist, K outside 2..64, a cls entry in [K, 254] (checked before
 * the walk), weights that do not cover the chromosome.
 * hh_tune("saddle_diag_tile", 64 .. HH_SADDLE_DIAG_TILE) lowers the number of
 * diagonals a wave of the expected sums owns, for the calls that follow. */
#define HH_SADDLE_DIAG_TILE 256
int hh_expected_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                       const double* weight, int64_t n_weight, int64_t lo, int64_t N, const uint8_t* bad,
                       int32_t ignore_diags, int64_t max_dist, double* sum, int64_t* nvalid,
                       int32_t on_device, void* stream);          /* sum, nvalid: max_dist + 1 entries */
int hh_saddle_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                     const double* weight, int64_t n_weight, int64_t lo, int64_t N, const uint8_t* bad,
                     const double* expected, const uint8_t* cls, int32_t K, int64_t min_dist, int64_t max_dist,
                     double* U, int64_t* Cu, int32_t on_device, void* stream);   /* U, Cu: K x K row-major */

/* ---------------------------------------------- pileups (aggregate analysis)
 *   hh_pileup_pixels   nothing: defined by this project
 * The sum of the observed or observed-over-expected (2 f + 1) x (2 f + 1)
 * windows around a list of features of one chromosome, straight from cooler's
 * pixel table.  Table, weight and validity conventions are exactly those of
 * hh_expected_pixels: global bins [lo, lo + N), unique pixels sorted by (bin1,
 * bin2) with bin1 <= bin2, a pixel with an end outside the chromosome is
 * ignored, v(a, b) = count * weight[bin1] * weight[bin2] in that order (NaN ->
 * 0; weight NULL: the raw count, else n_weight >= lo + N), valid[a] = 0 where
 * a weight is given and not finite or bad[a] != 0 (bad: uint8[N] or NULL);
 * nnz = 0 is valid.
 * Features k = 0 .. M - 1 have chromosome-local centres (row[k], col[k]), 0 <=
 * row[k] <= col[k] < N, in any order, repeats and overlaps allowed; row = col
 * is an on-diagonal feature.  flank f in 0..63, W = 2 f + 1.  Window cell (u,
 * v) of feature k is cell i = row[k] - f + u, j = col[k] - f + v of the
 * symmetric matrix, a = min(i, j), b = max(i, j), d = b - a; it is eligible
 * when 0 <= i, j < N, valid[i] and valid[j], d >= min_dist and, where expected
 * (double[n_expected], 1 <= n_expected <= N) is given, d < n_expected and
 * expected[d] is finite and > 0.  A window that leaves the chromosome is not
 * an error.  Outputs, W x W row-major: Cn[u][v] (int64) the features whose
 * cell (u, v) is eligible, stored or not; S[u][v] (fp64) the sum of t = v(a,
 * b), with expected t = v(a, b) / expected[d] (one IEEE division), over the
 * features whose cell is eligible and stored.  The order is fixed: chunks of
 * C = HH_PILEUP_CHUNK consecutive features are summed in ascending k from
 * +0.0, then the chunk sums in ascending chunk order from +0.0; products and
 * the division are never contracted into the additions and no floating-point
 * atomic is used, so two calls, the host and the device form and every grid
 * give the same bits.  hh_tune("pileup_chunk", 1 .. HH_PILEUP_CHUNK) lowers C
 * for the calls that follow (and with it the last bits).  M = 0 gives S = 0,
 * Cn = 0.  Every index derived from the table or from a feature is
 * range-checked before it addresses anything: a malformed table may give
 * wrong numbers, never an out-of-range access.
 * on_device: the table, weight, bad, row, col, expected and the outputs are
 * device pointers; otherwise host pointers.  HH_ERR_ARG (outputs untouched):
 * N < 1, flank outside 0..63, min_dist < 0, n_expected outside 1..N with an
 * expected, a feature with row > col or an end outside [0, N) (checked before
 * the walk; in the device form on the device), weights that do not cover the
 * chromosome. */
#define HH_PILEUP_CHUNK 64
int hh_pileup_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                     const double* weight, int64_t n_weight, int64_t lo, int64_t N, const uint8_t* bad,
                     const int32_t* row, const int32_t* col, int64_t M, int32_t flank,
                     const double* expected, int64_t n_expected, int64_t min_dist,
                     double* S, int64_t* Cn, int32_t on_device, void* stream);   /* S, Cn: W x W row-major */

/* ------------------------------------ domain pileups (rescaled aggregate)
 *   hh_domain_pileup_pixels   nothing: defined by this project
 * The sum of the observed or observed-over-expected maps of a list of
 * intervals (domains) of unequal size, each stretched to the same G x G grid,
 * straight from cooler's pixel table.  Table, weights, validity, bad,
 * expected, min_dist and the eligibility of a matrix cell (i, j) are exactly
 * hh_pileup_pixels': the cell is eligible when 0 <= i, j < N, both bins are
 * valid, d = |i - j| >= min_dist and, with an expected, d < n_expected and
 * expected[d] is finite and > 0; t = v(a, b) = count * weight[bin1] *
 * weight[bin2] in that order (NaN -> 0), over expected[d] as one IEEE division.
 * Feature k = 0 .. M - 1 is the half-open interval [start[k], end[k]) of
 * local bins, 0 <= start < end <= N, L = end - start; any order, repeats and
 * overlaps allowed.  R >= 1 output cells span the body, P >= 0 cells of flank
 * lie on each side, G = R + 2 P <= 127; every output cell spans L / R bins.
 * All geometry is 64-bit integer in units of 1/R bin: output index u covers
 * [start R + (u - P) L, start R + (u - P + 1) L), bin i covers [i R, (i + 1)
 * R), o(u, i) is the length of their intersection (0 .. min(L, R)).  A flank
 * may leave the chromosome: its cells are not eligible.
 * Upper form: output cell (u, v), u <= v, takes the matrix cells a <= b with
 * the integer weight c = o(u, a) o(v, b), doubled where a != b and u == v (the
 * mirrored cell (b, a) lands in the same output cell); the lower triangle is
 * the mirror, so S and Wn are symmetric bit for bit.
 *   A_k(u, v)  the exact int64 sum of c over the eligible cells, stored or not;
 *   T_k(u, v)  the sum of t * phi over the eligible stored cells, phi =
 *              double(c) / double(L L) (one IEEE division of two exact
 *              integers), from +0.0 in ascending (a, b) -- the order of the
 *              table; nothing is contracted;
 *   S  = sum_k T_k,  Wn = sum_k double(A_k) / double(L_k L_k), G x G row-major
 * fp64, both in hh_pileup_pixels' order across features: chunks of C =
 * HH_PILEUP_CHUNK (hh_tune "pileup_chunk") consecutive k in ascending k from
 * +0.0, then the chunk sums in ascending chunk order from +0.0.  No
 * floating-point atomic is used: two calls, the host and the device form and
 * every grid give the same bits.  A feature has weight 1 in a cell it covers
 * with eligible bins only; the pileup is S / Wn.  With L == R for every
 * feature and G odd, S and Wn equal hh_pileup_pixels' S and Cn for row = col =
 * start - P + (G - 1) / 2, flank (G - 1) / 2.  M = 0 gives zeros.  Every index
 * derived from the table or from a feature is range-checked before it
 * addresses anything: a malformed table may give wrong numbers, never an
 * out-of-range access.
 * on_device: the table, weight, bad, start, end, expected and the outputs are
 * device pointers; otherwise host pointers.  HH_ERR_ARG (outputs untouched):
 * N < 1, R < 1, P < 0, G > 127, min_dist < 0, n_expected outside 1..N with an
 * expected, a feature with start < 0, end > N or start >= end (checked before
 * the walk; in the device form on the device), weights that do not cover the
 * chromosome. */
int hh_domain_pileup_pixels(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                            const double* weight, int64_t n_weight, int64_t lo, int64_t N, const uint8_t* bad,
                            const int32_t* start, const int32_t* end, int64_t M, int32_t R, int32_t P,
                            const double* expected, int64_t n_expected, int64_t min_dist,
                            double* S, double* Wn, int32_t on_device, void* stream);   /* S, Wn: G x G row-major */

/* ------------------------- reproducibility (stratum-adjusted correlation)
 *   hh_scc_pixels   nothing: defined by this project
 * The per-stratum moments of two smoothed maps of the same chromosome,
 * straight from two pixel tables: table A covers global bins [lo_a, lo_a + N)
 * of its file, table B [lo_b, lo_b + N) of its own (the two differ for the M
 * and P copy inside one haplotype cooler).  Table, weight and validity
 * conventions of either side are exactly those of hh_expected_pixels: unique
 * pixels sorted by (bin1, bin2) with bin1 <= bin2, a pixel with an end outside
 * the chromosome is ignored, v(a, b) = (count * weight[bin1]) * weight[bin2]
 * (NaN -> 0; weight NULL: the raw count, else n_weight >= lo + N), valid_x[j] =
 * 0 where a weight is given and not finite or bad_x[j] != 0 (bad: uint8[N] or
 * NULL); nnz = 0 on either side is valid.  valid = valid_a & valid_b.
 * x(a, b) is the symmetric value of A, 0 where a or b is not valid or |a - b|
 * < ignore_diags; y(a, b) the same of B.  With half-width h in 0 ..
 * HH_SCC_MAX_H: SX(a, b) = the sum of x(a + p, b + q) over |p|, |q| <= h inside
 * [0, N)^2, by plain additions (no sliding add-and-subtract), nv(a) = the
 * valid bins among a - h .. a + h inside [0, N), X(a, b) = SX(a, b) / (nv(a)
 * nv(b)) (an exact integer product, one IEEE division); SY, Y from B.  For a
 * stratum d in [ignore_diags, max_dist] the cells are a in [0, N - d) with
 * valid[a] and valid[a + d], except those with SX(a, a + d) == 0 and SY(a, a +
 * d) == 0; n[d] (int64) counts them and S (5 x (max_dist + 1), row-major)
 * holds the fp64 sums of X, Y, X^2, Y^2 and X Y over them.  Below
 * ignore_diags n and S are 0.  The correlations are host work (DESIGN.md
 * §4q).
 * The sums have an order fixed by the tables, h and hh_tune("scc_rows"), the
 * two tables go through the same instructions, products are never contracted
 * into the additions and no floating-point atomic is used: two calls and the
 * host and the device form give the same bits, and swapping A and B gives the
 * same bits with Sx / Sy and Sxx / Syy swapped; n is exact.
 * hh_tune("scc_rows", 4 .. 32 in steps of 4; 0: chosen from h) sets the rows
 * of a work item for the calls that follow (and with it the last bits where
 * the arithmetic is not exact).  Every index derived from a table is
 * range-checked before it addresses anything: a malformed table may give
 * wrong numbers, never an out-of-range access.
 * on_device: the tables, weights, bad lists and the outputs are device
 * pointers; otherwise host pointers.  HH_ERR_ARG (outputs untouched): N < 1 or
 * N > 2^24, h outside 0 .. HH_SCC_MAX_H, ignore_diags < 0, max_dist outside
 * [0, N - 1], weights that do not cover the chromosome, null outputs. */
#define HH_SCC_MAX_H 20
int hh_scc_pixels(const int64_t* bin1_a, const int64_t* bin2_a, const double* count_a, int64_t nnz_a,
                  const double* weight_a, int64_t n_weight_a, int64_t lo_a, const uint8_t* bad_a,
                  const int64_t* bin1_b, const int64_t* bin2_b, const double* count_b, int64_t nnz_b,
                  const double* weight_b, int64_t n_weight_b, int64_t lo_b, const uint8_t* bad_b,
                  int64_t N, int32_t h, int32_t ignore_diags, int64_t max_dist,
                  int64_t* n, double* S /* 5 x (max_dist + 1), row-major: Sx Sy Sxx Syy Sxy */,
                  int32_t on_device, void* stream);

/* --------------------- trans expected, cis / trans totals and trans saddle
 *   hh_trans_blocks / hh_trans_saddle   nothing: defined by this project
 *                                       
 * The pair-of-chromosomes interface.  The genome is C chromosomes, 1 <= C <=
 * HH_TRANS_MAX_CHROMS; chrom_offset is int64[C + 1], strictly ascending from
 * chrom_offset[0] = 0 to chrom_offset[C] = n_bins, and c(x) is the chromosome
 * of global bin x.  use is uint8[C] or NULL (all): a chromosome with use = 0
 * contributes nothing, as a row or as a column.  chrom_offset and use are
 * host arrays in either form of the call (they are arguments, not data).
 * The pixels are cooler's: unique, bin1 <= bin2, global ids, sorted by (bin1,
 * bin2); v(a, b) = count * weight[a] * weight[b] in that order, NaN -> 0
 * (weight NULL: the raw count; n_weight >= n_bins otherwise).  valid[x] = 0
 * where use[c(x)] = 0, or a weight is given and weight[x] is not finite, or
 * bad[x] != 0; bad is uint8[n_bins], GLOBAL (the cis calls take the
 * chromosome's slice), or NULL.
 * One call handles the rows of one chromosome p: the pixels with
 * chrom_offset[p] <= bin1 < chrom_offset[p + 1].  Pixels with bin1 outside
 * are ignored, so the whole table and a slice that holds those rows give the
 * same result, bit for bit.  nnz = 0 is valid.
 * hh_trans_blocks: sum is fp64[C], npix int64[C].  For q > p sum[q] is the
 * fp64 sum of v(a, b) over the stored pixels with a in p, b in q and both
 * bins valid, npix[q] their number (a stored count of 0 counts); for q = p
 * the same over the pixels with b - a >= ignore_diags; for q < p both are 0.
 * The trans expected of a block is sum / (valid bins of p x valid bins of q),
 * host arithmetic.
 * hh_trans_saddle: cls is uint8[n_bins], global, class ids 0 .. K - 1 or 255
 * for a bin left out, 2 <= K <= 64; expected is double[C], row p of the trans
 * expected.  Block (p, q) is usable when q > p and expected[q] is finite and
 * > 0.  Every stored pixel with a in p, b in q, (p, q) usable, both bins valid
 * and both classes != 255 adds v(a, b) / expected[q] (an IEEE division) to
 * U[cls[a] * K + cls[b]]; U is K x K fp64, row-major.  The cell counts need no
 * pixel and are host integer arithmetic.
 * Order of the sums.  hh_trans_blocks: the pixels of the rows of p, counted
 * from the first of them, are cut into spans of 64 T pixels, T =
 * hh_tune("trans_trips", 1 .. HH_TRANS_MAX_TRIPS; default HH_TRANS_TRIPS), and
 * a span into trips of 64;
 * inside a trip the pixels of one (row, partner q) are consecutive and are
 * summed by a segmented Hillis-Steele scan over the 64 positions (a pixel left
 * out enters as +0.0); the segment sums are added to the span's acc[q] in
 * table order from +0.0; the span sums are added in groups of 64 consecutive
 * spans in ascending order from +0.0, the group sums likewise, until one sum
 * is left (a 64-ary tree fixed by the number of spans).  trans_trips changes the last bits of sum where the arithmetic
 * is not exact (npix never).  hh_trans_saddle: a row's trans pixels are added
 * per class of b in table order, the rows per class of a in ascending a
 * inside chunks of 512 rows, the chunks in ascending order; no tuning key
 * touches it.  Products and the division are never contracted into the
 * additions and no floating-point atomic is used: two calls, the host and the
 * device form and every grid give the same bits.  Every index derived from
 * the table (the pixel range of p, the row pointers, bin1, bin2, the partner
 * chromosome, the class) is range-checked before it addresses anything: a
 * malformed table may give wrong numbers, never an out-of-range access.
 * on_device: bin1 / bin2 / count / weight / bad / expected / cls and the
 * outputs are device pointers; otherwise host pointers.  HH_ERR_ARG (outputs
 * untouched): C outside 1 .. HH_TRANS_MAX_CHROMS, offsets not strictly
 * ascending or not starting at 0, p outside [0, C), a chromosome p of more
 * than 2^24 bins, ignore_diags < 0, K outside 2..64, a cls entry in [K, 254]
 * (checked before the walk), weights that do not cover n_bins, null pixel
 * arrays with nnz > 0. */
#define HH_TRANS_MAX_CHROMS 512
#define HH_TRANS_TRIPS 8
#define HH_TRANS_MAX_TRIPS 256
int hh_trans_blocks(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                    const double* weight, int64_t n_weight, const int64_t* chrom_offset, int32_t C,
                    const uint8_t* use, const uint8_t* bad, int32_t p, int32_t ignore_diags,
                    double* sum, int64_t* npix, int32_t on_device, void* stream);   /* sum, npix: C entries */
int hh_trans_saddle(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                    const double* weight, int64_t n_weight, const int64_t* chrom_offset, int32_t C,
                    const uint8_t* use, const uint8_t* bad, int32_t p, const double* expected,
                    const uint8_t* cls, int32_t K, double* U, int32_t on_device, void* stream);   /* U: K x K row-major */

/* ------------------------- the symmetric trans operator (trans eigenvectors)
 *   hh_teig_*   nothing: defined by this project
 * The genome (chrom_offset, C, use), the pixels, v(a, b) = count * weight[a] *
 * weight[b] (in that order, NaN -> 0), bad and valid[x] are hh_trans_*'s,
 * word for word; n_bins < 2^31.  T is the symmetric n_bins x n_bins matrix
 * with T[i][j] = v(min(i, j), max(i, j)) where i and j are valid and on
 * different chromosomes and the pixel is stored, 0 elsewhere (the cis blocks
 * are empty).
 * hh_teig_create stages the table (on_device: bin1 / bin2 / count / weight /
 * bad are device pointers and are not needed after the call returns) and
 * builds two trans-only row-compressed tables, each int64 row pointers
 * [n_bins + 1], int32 partners and fp64 values v: `upper` (row bin1, partners
 * bin2 ascending) and `lower`, its transpose (row bin2, partners bin1
 * ascending).  Pixels inside a chromosome or with an invalid end are dropped
 * and v is computed once, here.  Both tables are pure functions of the input:
 * the upper one is the table compacted in its own order, the lower one a
 * stable radix sort of (bin2, slot in the upper table); no cursor, no timing.
 * C = 1, nnz = 0 or no kept pixel give empty tables, not an error.
 * hh_teig_nnz: the entries of either table (equal).  hh_teig_export(which = 0
 * upper / 1 lower) downloads one table to host arrays (tests).
 * hh_teig_apply: Y = D T (D X), X and Y n_bins x k fp64 row-major, 1 <= k <=
 * HH_TEIG_MAX_K, d fp64[n_bins] or NULL (all ones); on_device: d, X, Y are
 * device pointers, otherwise host pointers.  Y[i][c] = d[i] * sum_j T[i][j] *
 * (d[j] * X[j][c]): the two scalings by d are IEEE multiplications of their
 * own.  Rows of invalid bins are +0.0 whatever d and X hold there.
 * Order of the sums.  One wave owns row i; position l of 64 adds the entries
 * l, l + 64, ... of the row's lower segment and then of its upper segment from
 * +0.0, in that order; the 64 partial sums are added by an xor butterfly
 * (distances 32, 16, 8, 4, 2, 1).  The order depends on the two tables alone:
 * not on the grid (hh_tune "teig_rows", rows per block, 1 .. HH_TEIG_MAX_ROWS,
 * default HH_TEIG_ROWS), not on k -- column c of a k = 8 call has the bits of
 * the k = 1 call on that column -- and not on the timing.  No product is
 * contracted into an addition and no floating-point atomic is used: two
 * calls, the host and the device form give the same bits.  Every bin id of
 * the table is compared with n_bins before it indexes anything; a malformed
 * table may give wrong numbers, never an out-of-range access.
 * The term M X of the operator E = D T D - M needs no pixel and is host
 * arithmetic (hichap_master_amd/transeig.py).
 * HH_ERR_ARG (outputs untouched): C outside 1 .. HH_TRANS_MAX_CHROMS, offsets
 * not strictly ascending or not starting at 0, n_bins >= 2^31, weights that do
 * not cover n_bins, null pixel arrays with nnz > 0; hh_teig_apply: k outside
 * 1 .. HH_TEIG_MAX_K, null X or Y, a d entry on a valid bin that is negative
 * or not finite (checked before Y is written). */
#define HH_TEIG_MAX_K 8
#define HH_TEIG_ROWS 4
#define HH_TEIG_MAX_ROWS 16
typedef struct hh_teig hh_teig;
int hh_teig_create(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                   const double* weight, int64_t n_weight, const int64_t* chrom_offset, int32_t C,
                   const uint8_t* use, const uint8_t* bad, int32_t on_device, void* stream, hh_teig** out);
int hh_teig_nnz(const hh_teig* h, int64_t* upper, int64_t* lower);
int hh_teig_export(const hh_teig* h, int32_t which, int64_t* rowptr, int32_t* partner, double* value);
int hh_teig_apply(const hh_teig* h, const double* d, const double* X, int32_t k, double* Y, int32_t on_device,
                  void* stream);
int hh_teig_free(hh_teig* h);

/* ------------- the symmetric pixel table: per-bin coverage and virtual 4C
 *   hh_symtab_*   nothing: defined by this project
 * The genome (chrom_offset, C, use), the pixels, v(a, b) = count * weight[a] *
 * weight[b] (in that order, NaN -> 0; weight NULL: the raw count), bad and
 * valid[x] are hh_trans_*'s, word for word; n_bins < 2^31, nnz < 2^32 (the
 * sort's offsets are 32-bit).  A is the symmetric n_bins x n_bins matrix with
 * A[i][j] = v(min(i, j), max(i, j)) where i and j are valid and the pixel is
 * stored, 0 elsewhere.  A diagonal pixel (i, i) enters row i ONCE.  With d =
 * |i - j| a cell is `trans` (different chromosomes), dropped (cis, d <
 * ignore_diags), `near` (cis, ignore_diags <= d < near_bins) or `far` (cis, d
 * >= max(near_bins, ignore_diags)); near_bins <= ignore_diags leaves `near`
 * empty.
 * hh_symtab_create stages the whole table (on_device: bin1 / bin2 / count are
 * device pointers; in either form they are not needed after the call returns)
 * and keeps, on the device: the upper table in its own order (int64 row
 * pointers rowptr_u[n_bins + 1], the lower bounds of bin1; int32 bin2, -1
 * where it is outside [0, n_bins); the fp64 counts), the chromosome of every
 * bin, and the lower table: every stored pixel with bin1 < bin2 and both ids
 * in [0, n_bins), sorted by (bin2, bin1): rowptr_l int64[n_bins + 1],
 * partner_l int32 (the pixel's bin1), src_l uint32 (its index in the upper
 * table) and a copy of its count.  The lower table is a stable radix sort of
 * the keys (bin2 << 33 | index) on the bin2 bits; a diagonal or out-of-range
 * pixel gets the key n_bins << 33 | index, sorts behind the last row and gets
 * no entry.  Nothing depends on weights or validity: one handle serves raw and
 * balanced calls and any use / bad.  C = 1 and nnz = 0 are valid and launch
 * nothing over an empty table.  hh_symtab_nnz: the entries of the upper table
 * (nnz) and of the lower one.  hh_symtab_export downloads the row pointers
 * and the lower table to host arrays (tests; partner_l / src_l may be NULL
 * where lower = 0).
 * hh_symtab_coverage: S is fp64[n_bins * 3], n int64[n_bins * 3], row-major,
 * the classes in the order near, far, trans.  S[x][k] is the sum of A[x][j]
 * over the cells of class k, n[x][k] the stored pixels behind it (a stored
 * count of 0 counts); an invalid x gets +0.0 and 0.
 * hh_symtab_viewpoints: viewpoint c is the half-open interval of global bins
 * [lo[c], hi[c]), lo and hi HOST int64[K] in either form, 1 <= K <=
 * HH_SYMTAB_MAX_VIEWS.  P is fp64[K * n_bins], viewpoint-major: P[c][y] = the
 * sum over the valid x in [lo[c], hi[c]) of A[x][y] without the dropped cells,
 * for a valid y; an invalid y gets +0.0.  An interval may cross a chromosome
 * end: the class is decided per cell.
 * Order of the sums.  Coverage: one wave owns bin x; position l of 64 takes
 * the entries l, l + 64, ... of the bin's lower segment and then of its upper
 * segment into three running sums from +0.0 (an entry of another class or with
 * an invalid partner adds nothing); the 64 partial sums of a class are added
 * by an xor butterfly (distances 32, 16, 8, 4, 2, 1).  Viewpoints: for a fixed
 * (c, y) the terms are added from +0.0 in ascending x: the entries of the
 * lower segment of y whose partner lies in [lo, hi) (a contiguous run, found
 * by two bisections), then those of the upper segment.  The orders depend on
 * the table and the arguments alone: not on the grid (hh_tune "cov_rows", bins
 * per block of the coverage walk, 1 .. HH_COV_MAX_ROWS, default HH_COV_ROWS),
 * not on K -- column c of a K = 64 call has the bits of the K =
 * 1 call -- and not on the timing.  No product is contracted into an addition
 * and no floating-point atomic is used: two calls, the host and the device
 * form give the same bits.  Every id read from a table (a partner, a
 * row pointer) is compared with n_bins or the table's length before it
 * indexes anything, and row pointers out of order make an empty row: a
 * malformed table (unsorted, bin1 > bin2, ids out of range) may give wrong
 * numbers, never an out-of-range access.
 * on_device: weight / bad and the outputs are device pointers; otherwise host
 * pointers; use, lo and hi are host arrays.  HH_ERR_ARG (outputs untouched):
 * hh_symtab_create: C outside 1 .. HH_TRANS_MAX_CHROMS, offsets not strictly
 * ascending or not starting at 0, n_bins >= 2^31, nnz < 0 or >= 2^32, null
 * pixel arrays with nnz > 0; the two calls: a null handle, ignore_diags < 0,
 * near_bins < 0, weights that do not cover n_bins, null outputs; K outside 1 ..
 * HH_SYMTAB_MAX_VIEWS, null lo or hi, lo[c] < 0, hi[c] > n_bins, lo[c] >=
 * hi[c]. */
#define HH_SYMTAB_MAX_VIEWS 64
#define HH_COV_ROWS 4
#define HH_COV_MAX_ROWS 16
typedef struct hh_symtab hh_symtab;
int hh_symtab_create(const int64_t* bin1, const int64_t* bin2, const double* count, int64_t nnz,
                     const int64_t* chrom_offset, int32_t C, int32_t on_device, void* stream, hh_symtab** out);
int hh_symtab_nnz(const hh_symtab* h, int64_t* upper, int64_t* lower);
int hh_symtab_export(const hh_symtab* h, int64_t* rowptr_u, int64_t* rowptr_l, int32_t* partner_l, uint32_t* src_l);
int hh_symtab_coverage(const hh_symtab* h, const double* weight, int64_t n_weight, const uint8_t* use,
                       const uint8_t* bad, int32_t ignore_diags, int32_t near_bins, double* S, int64_t* n,
                       int32_t on_device, void* stream);   /* S, n: n_bins x 3 row-major (near, far, trans) */
int hh_symtab_viewpoints(const hh_symtab* h, const double* weight, int64_t n_weight, const uint8_t* use,
                         const uint8_t* bad, int32_t ignore_diags, const int64_t* lo, const int64_t* hi, int32_t K,
                         double* P, int32_t on_device, void* stream);   /* P: K x n_bins row-major */
int hh_symtab_free(hh_symtab* h);

#ifdef __cplusplus
}
#endif
#endif /* HICHAP_HIP_H */
