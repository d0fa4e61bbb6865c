// The decisions of the linkage's host side (fluidaudio_amd/csrc/ahc_route.h: what ahc_rounds_host.hip and ahc_batch_host.hip choose slots per thread,
// kernels, budgets and the batch route with) driven over stdin: one command per line.
// Test infrastructure: built by tests/test_ahc_route.py with g++ and the address / undefined-behaviour sanitizers, no GPU.
//   single forced no_single_block N        -> "cpt Np blocks fits"
//   form cpt nblk mode d spec_on           -> "big kc spec kernel"
//   rounds N                               -> "rounds budget"
//   elig mode no_uniform count n...        -> "0" or "1"
//   ucpt forced count Nmax                 -> slots per thread of the uniform batch
//   groups forced count n...               -> uniform batches side by side
//   ukern cpt nblk waves                   -> the uniform kernel
//   route mode allow_groups capped in_flight forced_groups no_uniform count n...  -> "route groups"
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fluidaudio_amd/csrc/ahc_route.h"

using namespace fa_ahc;

static const char *single_name(const route::SingleKernel k) {
    switch (k) {
        case route::kSpecK1: return "spec_k1"; case route::kSpecK2: return "spec_k2"; case route::kSpecK3: return "spec_k3"; case route::kSpecK4: return "spec_k4";
        case route::kC4Big: return "c4_big"; case route::kC4: return "c4"; case route::kC2Big: return "c2_big"; case route::kC2: return "c2";
        case route::kC1Big: return "c1_big"; case route::kC1K1: return "k1"; case route::kC1K2: return "k2"; case route::kC1K3: return "k3"; case route::kC1K4: return "k4";
        default: return "?";
    }
}
static const char *uni_name(const route::UniKernel k) {
    switch (k) {
        case route::kUni: return "uni"; case route::kUniW3: return "uni_w3"; case route::kUniW4: return "uni_w4"; case route::kUniC2: return "uni_c2";
        case route::kUniC4: return "uni_c4"; case route::kUniK1: return "uni_k1"; case route::kUniK2: return "uni_k2"; case route::kUniK3: return "uni_k3";
        case route::kUniC2K1: return "uni_c2k1";
        default: return "?";
    }
}
static const char *route_name(const route::Route r) {
    switch (r) {
        case route::Route::kOversize: return "oversize"; case route::Route::kGroups: return "groups"; case route::Route::kInFlight: return "in_flight";
        case route::Route::kUniform: return "uniform"; case route::Route::kBlockMap: return "block_map";
    }
    return "?";
}
static bool read_sizes(std::vector<size_t> &n) {   // "count n...": exactly count sizes, so that the sanitizers watch the reads
    int count;
    if (scanf("%d", &count) != 1 || count < 0) return false;
    n.assign(static_cast<size_t>(count), 0);
    for (size_t &x : n) if (scanf("%zu", &x) != 1) return false;
    return true;
}

int main() {
    char cmd[16];
    std::vector<size_t> n;
    while (scanf("%15s", cmd) == 1) {
        int a, b, c, e, f, g;
        size_t N;
        if (!strcmp(cmd, "single")) {
            if (scanf("%d %d %zu", &a, &b, &N) != 3) return 2;
            const int cpt = route::single_cpt(a, b != 0, N);
            printf("%d %zu %zu %d\n", cpt, route::padded(N, cpt), route::blocks(N, cpt), route::fits_matrix(N) ? 1 : 0);
        } else if (!strcmp(cmd, "form")) {
            if (scanf("%d %d %d %zu %d", &a, &b, &c, &N, &e) != 5) return 2;
            const route::RoundForm fm = route::single_form(a, b, c, N, e != 0);
            printf("%d %d %d %s\n", fm.big ? 1 : 0, fm.kc, fm.spec ? 1 : 0, single_name(fm.kernel));
        } else if (!strcmp(cmd, "rounds")) {
            if (scanf("%zu", &N) != 1) return 2;
            printf("%d %lld\n", route::rounds_for(N), route::replay_budget(N));
        } else if (!strcmp(cmd, "elig")) {
            if (scanf("%d %d", &a, &b) != 2 || !read_sizes(n)) return 2;
            printf("%d\n", route::uniform_eligible(static_cast<int>(n.size()), n.data(), a, b != 0) ? 1 : 0);
        } else if (!strcmp(cmd, "ucpt")) {
            if (scanf("%d %d %zu", &a, &b, &N) != 3) return 2;
            printf("%d\n", route::uniform_cpt(a, b, N));
        } else if (!strcmp(cmd, "groups")) {
            if (scanf("%d", &a) != 1 || !read_sizes(n)) return 2;
            printf("%d\n", route::uniform_groups(static_cast<int>(n.size()), n.data(), a));
        } else if (!strcmp(cmd, "ukern")) {
            if (scanf("%d %d %d", &a, &b, &c) != 3) return 2;
            printf("%s\n", uni_name(route::uniform_kernel(a, b, c)));
        } else if (!strcmp(cmd, "route")) {
            if (scanf("%d %d %d %d %d %d", &a, &b, &c, &e, &f, &g) != 6 || !read_sizes(n)) return 2;
            const route::BatchRoute r = route::batch_route(static_cast<int>(n.size()), n.data(), a, b != 0, c != 0, e != 0, f, g != 0);
            printf("%s %d\n", route_name(r.route), r.groups);
        } else {
            return 2;
        }
    }
    return 0;
}
