// CPU walk of the edit-distance kernel's schedule (fluidaudio_amd/csrc/wer.hip) over the code it shares with the host: the cell and the
// strip row of wer_core.h, the plan, the boundary layout and the answer's place of wer_launch.h.  64 emulated lanes per pair, strips of
// C columns, rows walked skewed, the left neighbour's cell and the hypothesis symbol handed over by a shift of one lane per step, lane
// 0 fed from 64-row blocks loaded one block ahead, panels chained through the boundary buffers.  The workspace starts poisoned and
// every entry remembers whether this run wrote it: reading one that was not written, or anything out of bounds, ends the program.
// Test infrastructure: built with g++ by tests/test_wer_emul.py, no GPU.
//   wer_emul < pairs     "n_pairs", then per pair "m n", m hypothesis symbols, n reference symbols
//   prints per pair      total insertions deletions substitutions hyp_len ref_len class panels
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../fluidaudio_amd/csrc/wer_core.h"
#include "../../fluidaudio_amd/csrc/wer_launch.h"

using fa::wer::Job;
using fa::wer::kWave;
using fa::wercore::Cell;

static void fail(const char *what) {
    std::fprintf(stderr, "wer_emul: %s\n", what);
    std::exit(3);
}

struct Workspace {
    std::vector<int32_t> v;
    std::vector<char> written;
    explicit Workspace(int64_t n) : v(static_cast<size_t>(n), -1), written(static_cast<size_t>(n), 0) {}
    void store(int64_t i, int32_t x) {
        if (i < 0 || i >= static_cast<int64_t>(v.size())) fail("store outside the workspace");
        v[static_cast<size_t>(i)] = x;
        written[static_cast<size_t>(i)] = 1;
    }
    int32_t load(int64_t i) const {
        if (i < 0 || i >= static_cast<int64_t>(v.size())) fail("load outside the workspace");
        if (!written[static_cast<size_t>(i)]) fail("load of a workspace entry this run did not write");
        return v[static_cast<size_t>(i)];
    }
};

// the wave shift: lane l gets lane l - 1's value, lane 0 the fill
template <class T>
static void below(const T (&v)[kWave], const T fill, T (&out)[kWave]) {
    for (int l = kWave - 1; l > 0; --l) out[l] = v[l - 1];
    out[0] = fill;
}

template <int C>
static void walk(const Job &job, const std::vector<int32_t> &hyp_all, const std::vector<int32_t> &ref_all, Workspace &ws, int32_t (&out)[4]) {
    const uint32_t m = static_cast<uint32_t>(job.m);
    const auto hyp = [&](const uint32_t r) {
        const int64_t i = job.hyp_off + r;
        if (r >= m || i >= static_cast<int64_t>(hyp_all.size())) fail("hypothesis read out of bounds");
        return hyp_all[static_cast<size_t>(i)];
    };
    const auto ref = [&](const int64_t c) {
        const int64_t i = job.ref_off + c;
        if (c >= job.n || i >= static_cast<int64_t>(ref_all.size())) fail("reference read out of bounds");
        return ref_all[static_cast<size_t>(i)];
    };
    static Cell strip[kWave][C];
    for (int32_t p = 0; p < job.panels; ++p) {
        const bool first = p == 0, last = p == job.panels - 1;
        static int32_t sym[kWave][C];
        Cell diag[kWave];
        for (int lane = 0; lane < kWave; ++lane) {
            const int64_t col0 = (static_cast<int64_t>(p) * kWave + lane) * C;
            for (int c = 0; c < C; ++c) {
                sym[lane][c] = col0 + c < job.n ? ref(col0 + c) : 0;
                strip[lane][c] = fa::wercore::row_zero(static_cast<int32_t>(col0 + c + 1));
            }
            diag[lane] = fa::wercore::row_zero(static_cast<int32_t>(col0));
        }
        const int64_t rd = job.ws_off + fa::wer::boundary_at(job.m, (p - 1) & 1, 0), wr = job.ws_off + fa::wer::boundary_at(job.m, p & 1, 0);
        const uint32_t steps = fa::wer::steps_of(job.m, job.n, C, last);
        int32_t tok_blk[kWave], tok_next[kWave], tok[kWave] = {};
        Cell bnd_blk[kWave], bnd_next[kWave];
        const auto load = [&](const uint32_t r0, int32_t (&t)[kWave], Cell (&b)[kWave]) {
            for (int lane = 0; lane < kWave; ++lane) {
                const uint32_t r = r0 + lane;
                t[lane] = r < m ? hyp(r) : 0;
                b[lane] = Cell{0, 0, 0};
                if (!first && r < m) b[lane] = Cell{ws.load(rd + r), ws.load(rd + m + r), ws.load(rd + 2 * static_cast<int64_t>(m) + r)};
            }
        };
        load(0, tok_next, bnd_next);
        for (uint32_t s0 = 0; s0 < steps; s0 += kWave) {
            for (int lane = 0; lane < kWave; ++lane) { tok_blk[lane] = tok_next[lane]; bnd_blk[lane] = bnd_next[lane]; }
            load(s0 + kWave, tok_next, bnd_next);
            const int t_end = static_cast<int>(steps - s0 < static_cast<uint32_t>(kWave) ? steps - s0 : kWave);
            for (int t = 0; t < t_end; ++t) {
                const uint32_t s = s0 + t;
                const Cell feed = first ? fa::wercore::col_zero(static_cast<int32_t>(s + 1)) : bnd_blk[t];
                int32_t tok_in[kWave];
                Cell last_cell[kWave], left[kWave];
                below(tok, tok_blk[t], tok_in);
                for (int lane = 0; lane < kWave; ++lane) { tok[lane] = tok_in[lane]; last_cell[lane] = strip[lane][C - 1]; }
                below(last_cell, feed, left);
                for (int lane = 0; lane < kWave; ++lane) {
                    const uint32_t r = s - static_cast<uint32_t>(lane);
                    if (r >= m) continue;
                    fa::wercore::strip_row<C>(strip[lane], sym[lane], tok[lane], diag[lane], left[lane]);
                    diag[lane] = left[lane];
                    if (!last && lane == kWave - 1) {
                        ws.store(wr + r, strip[lane][C - 1].dp);
                        ws.store(wr + m + r, strip[lane][C - 1].sub);
                        ws.store(wr + 2 * static_cast<int64_t>(m) + r, strip[lane][C - 1].del);
                    }
                }
            }
        }
    }
    const Cell res = strip[fa::wer::last_lane(job.n, C)][fa::wer::last_slot(job.n, C)];
    out[0] = res.dp;
    out[1] = res.dp - res.sub - res.del;
    out[2] = res.del;
    out[3] = res.sub;
}

int main() {
    long long n_pairs = 0;
    if (std::scanf("%lld", &n_pairs) != 1 || n_pairs < 0) fail("bad input");
    std::vector<int32_t> hyp, ref;
    std::vector<int64_t> hyp_range{0}, ref_range{0};
    for (long long k = 0; k < n_pairs; ++k) {
        long long m = 0, n = 0, x = 0;
        if (std::scanf("%lld %lld", &m, &n) != 2 || m < 0 || n < 0) fail("bad input");
        for (long long i = 0; i < m; ++i) { if (std::scanf("%lld", &x) != 1) fail("bad input"); hyp.push_back(static_cast<int32_t>(x)); }
        for (long long i = 0; i < n; ++i) { if (std::scanf("%lld", &x) != 1) fail("bad input"); ref.push_back(static_cast<int32_t>(x)); }
        hyp_range.push_back(static_cast<int64_t>(hyp.size()));
        ref_range.push_back(static_cast<int64_t>(ref.size()));
    }
    if (n_pairs == 0) return 0;
    const fa::wer::Verdict v = fa::wer::check_ranges(hyp.data(), hyp_range.data(), ref.data(), ref_range.data(), n_pairs);
    if (v.status != FA_SUCCESS) fail(v.what);
    std::vector<fa_edit_counts> out(static_cast<size_t>(n_pairs));
    fa::wer::Plan plan;
    fa::wer::make_plan(hyp_range.data(), ref_range.data(), n_pairs, 0, 0, out.data(), plan);
    Workspace ws(plan.ws_ints);
    size_t base = 0;
    for (int c = 0; c < fa::wer::kClasses; ++c) {
        for (size_t i = base; i < base + static_cast<size_t>(plan.n_class[c]); ++i) {
            const Job &job = plan.jobs[i];
            if (fa::wer::class_of(job.n) != c) fail("a job is listed under another class");
            int32_t got[4];
            switch (c) {
            case 0: walk<1>(job, hyp, ref, ws, got); break;
            case 1: walk<2>(job, hyp, ref, ws, got); break;
            case 2: walk<4>(job, hyp, ref, ws, got); break;
            case 3: walk<8>(job, hyp, ref, ws, got); break;
            default: walk<16>(job, hyp, ref, ws, got); break;
            }
            fa_edit_counts &o = out[static_cast<size_t>(job.pair)];
            o.total = got[0]; o.insertions = got[1]; o.deletions = got[2]; o.substitutions = got[3];
        }
        base += static_cast<size_t>(plan.n_class[c]);
    }
    if (base != plan.jobs.size()) fail("the class counts do not add up to the job list");
    for (long long k = 0; k < n_pairs; ++k) {
        const fa_edit_counts &o = out[static_cast<size_t>(k)];
        const int32_t n = o.ref_len;
        std::printf("%d %d %d %d %d %d %d %d\n", o.total, o.insertions, o.deletions, o.substitutions, o.hyp_len, o.ref_len, fa::wer::class_of(n), fa::wer::panels_of(n));
    }
    return 0;
}
