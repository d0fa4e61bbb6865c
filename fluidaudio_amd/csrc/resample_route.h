// resample_route.h — which kernel family serves a fa_resample_poly_dev call, as plain C++ (no HIP types: tests/cpu/resample_routes.cpp walks it on
// the CPU): the facts of a rate pair's plan the choice reads, the switches of the tests, and the choice itself.  Part of resample_host.hip, which
// keeps the facts with the context's plan and launches what pick_route says; the geometry is resample_geom.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "resample_geom.h"

namespace fa {
namespace resample {

// What pick_route reads of a plan: the pair, its filter, and which families have an instance for it.
struct PlanFacts {
    int up = 0, down = 0;                       // reduced by their greatest common divisor
    int64_t n_taps = 0, pre_remove = 0;         // fa_resample_poly_taps
    bool decim_tiles = false, decim_regs = false, interp = false;   // poly_decim_tile_kernel / poly_decim_kernel / poly_interp_kernel have an instance
    bool has_rows = false;                      // the row tables are on the device: a row kernel serves the pair ...
    PolyRowsGeom rows_geom{};                   // ... with this geometry ...
    int tile_rows = 64;                         // ... and tiles of this many rows (64: poly_rows_kernel; 16 / 32: a wide kernel)
    size_t lds_bytes = 0;                       // what poly_lds_kernel needs for the pair: served up to kLdsLimit
};
constexpr size_t kLdsLimit = 150 * 1024;

// The kernel-choice switches of the tests, read ONCE per call (the forms fixed with a plan's tables — FA_RESAMPLE_WIDE, _NO_WIDE — are read when it is built).
struct Switches { bool simple, no_decim, no_decim_tiles, no_rows; };
// One family serves the interior outputs [lo, hi), poly_kernel the edges [0, lo) and [hi, n_out).  DECIM: tiles on [lo, split), the register-tiled kernel on
// [split, hi).  INTERP: `count` threads from phase cycle `split` on.  ROWS: `count` tiles.  LDS: everything.  SIMPLE: nothing — all outputs are edges.
enum class Kind { DECIM, INTERP, ROWS, LDS, SIMPLE };
struct Route { Kind kind; int64_t lo, hi, split, count; };

// The first family, in this order, that has an instance for the pair, is not switched off and finds whole work items inside the signal.
inline Route pick_route(const PlanFacts &P, const Switches &sw, const uintptr_t x_addr, const uintptr_t y_addr, const int64_t frames, const int64_t n_out) {
    if (sw.simple) return {Kind::SIMPLE, 0, 0, 0, 0};
    if (P.decim_tiles && !sw.no_decim && (x_addr & 15) == 0 && (y_addr & 7) == 0) {   // 16-byte loads, 8-byte stores
        fa::DecimSplit s = fa::decim_split(P.down, frames, n_out, !sw.no_decim_tiles);
        if (!P.decim_regs) s.m_regs = s.m_tiles;         // (192 kHz has tiles only: what they leave goes to the edges)
        if (s.m_regs > s.m_begin) return {Kind::DECIM, s.m_begin, s.m_regs, s.m_tiles, 0};
    }
    if (P.interp) {
        int64_t m_begin = 0, q_begin = 0, groups = 0;
        fa::interp_geometry(P.up, P.down, static_cast<int>(P.n_taps), fa::kInterpR, frames, n_out, P.pre_remove, m_begin, q_begin, groups);
        if (groups > 0) return {Kind::INTERP, m_begin, m_begin + groups * fa::kInterpR * P.up, q_begin, groups};
    }
    if (P.has_rows && !sw.no_rows) {
        const fa::PolyRowsGeom &G = P.rows_geom;
        const int64_t tiles = fa::rows_tiles(G, frames, n_out, P.tile_rows);       // tiles whose staged inputs all exist
        if (tiles > 0 && (tiles + 8) * G.groups < (1LL << 31)) return {Kind::ROWS, G.m_begin, std::min(n_out, G.m_begin + tiles * P.tile_rows * G.up), 0, tiles};
    }
    if (P.lds_bytes <= kLdsLimit) return {Kind::LDS, 0, n_out, 0, 0};
    return {Kind::SIMPLE, 0, 0, 0, 0};                   // very long filters (extreme rate ratios)
}

}  // namespace resample
}  // namespace fa
