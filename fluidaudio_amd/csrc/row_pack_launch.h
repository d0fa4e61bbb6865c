// row_pack_launch.h — the host side of "ragged rows from by-value groups": the operands of up to kGroup rows travel in one launch's
// arguments, so nothing is staged and no device entry waits.  Group is the row pack's operand (kernel and launcher: row_pack.h);
// for_each_group is the loop "fill a group, launch it, advance", also for a unit's own group types (fsmn_vad_launch.h: FeatGroup,
// GatherGroup).  Plain C++.  Users: tdt_plan_host.hip, sortformer_stream_host.hip, fsmn_vad_host.hip.
#pragma once
#include <algorithm>
#include <cstdint>

namespace fa {
namespace rows {

constexpr int kGroup = 64;                   // rows whose sources travel in one launch's arguments
constexpr int kPackSlice = 4096;             // elements of a row one workgroup writes

struct Group {                               // up to kGroup rows, by value in the launch's arguments: no table to upload
    int64_t src[kGroup];                     // the row's first element, from the array the kernel is given
    int32_t len[kGroup];                     // elements copied; zeros behind them
    int32_t count;
};

// Items [0, n) in groups of kGroup: fill(g, i, k) sets slot k of the group from item i, launch(g, first) issues the group whose slot 0 is
// item `first`.  G: a struct of per-slot arrays and an int32 `count`.
template <class G = Group, class Fill, class Launch>
inline void for_each_group(const int64_t n, const Fill &fill, const Launch &launch) {
    for (int64_t first = 0; first < n; first += kGroup) {
        G g{};
        g.count = static_cast<int32_t>(std::min<int64_t>(kGroup, n - first));
        for (int32_t k = 0; k < g.count; ++k) fill(g, first + k, k);
        launch(g, first);
    }
}

}  // namespace rows
}  // namespace fa
