// resample_launch.h — what the resampler's host code (resample_host.hip: taps, tables, the per-context plan, the route of a call, the C ABI) and
// its kernel translation unit (resample.hip) share: one call's operands, the row tables of a rate pair, and one launcher per family of polyphase kernels with
// the query that says whether the family has an instance for a pair.  Template arguments are named in resample.hip only.  Internal; not part
// of the C ABI.  Everything is enqueued on Job::stream; launch errors surface through hipGetLastError().
#pragma once
#include "fa_common.h"
#include "resample_geom.h"

namespace fa {
namespace resample {

struct Job {   // one fa_resample_poly_dev call: x (frames samples) -> y (n_out samples) through the pair's taps h
    hipStream_t stream;
    const float *x, *h;
    float *y;
    int64_t frames, n_out, n_taps, pre_remove;
    int up, down;
};

// The tables of poly_rows_kernel / the wide kernels for one rate pair (fa::rows_geometry), resident on the device; the plan owns d_tables.
struct RowsTables {
    bool wide = false;              // served by a wide kernel (16- or 32-row tiles, persistent workgroups, two LDS buffers)
    int wide_rows = 0, wide_waves = 0, ch = 0;   // its rows per tile (32: units of 8 phases, 16: of 16); wavefronts per workgroup; units per wavefront
    PolyRowsGeom g{};
    int nv = 0;                     // 16-byte reads per phase window
    void *d_tables = nullptr;       // [gtab int2 x groups, padded to 256 B][table rows: kRowsTT floats per phase]; null: the pair has no row tables
    size_t tt_offset = 0;
    int tile_rows() const { return wide ? wide_rows : 64; }
};

// poly_kernel, one thread per output, on the outputs [m_lo, m_hi): any pair, clamps at the signal's ends (the edges of every other route)
void launch_edges(const Job &j, int64_t m_lo, int64_t m_hi);
// poly_lds_kernel on every output: any pair whose taps + the input span of a tile fit the LDS (lds_need: their bytes)
size_t lds_need(int up, int down, int64_t n_taps);
void launch_lds(const Job &j, size_t lds_bytes);
// integer decimation (fa::decim_split): poly_decim_tile_kernel<down> on the outputs [m_begin, m_end), poly_decim_kernel<down> on [m_begin, m_end)
bool decim_tiles_instance(int down);
bool decim_instance(int down);
void launch_decim_tiles(int down, const Job &j, int64_t m_begin, int64_t m_end);
void launch_decim(int down, const Job &j, int64_t m_begin, int64_t m_end);
// poly_interp_kernel<up, down, n_taps> on `groups` threads from output m_begin / phase cycle q_begin on (fa::interp_geometry with fa::kInterpR)
bool interp_instance(int up, int down, int64_t n_taps);
void launch_interp(const Job &j, int64_t m_begin, int64_t q_begin, int64_t groups);
// poly_rows_kernel (one 64-row tile per workgroup) / the wide kernels on `tiles` tiles, outputs below m_end
bool rows_instance(int nv);
// a wide kernel for tiles of `rows` rows and `waves` wavefronts: rows of sld floats in `groups` phase groups, windows of nv reads shared by `share` phases, ch units per wavefront
bool wide_instance(int rows, int waves, int nv, int share, int ch, int sld, int groups);
void launch_rows(const Job &j, const RowsTables &t, int64_t tiles, int64_t m_end);
void launch_rows_wide(const Job &j, const RowsTables &t, int64_t tiles, int64_t m_end);

}  // namespace resample
}  // namespace fa
