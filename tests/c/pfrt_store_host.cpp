// Stand-alone host program (its own main, no GPU, no Python): the bookkeeping of the PFRT step store -- begin, record, the step
// loop's offsets -- driven through csrc/pfrt_store.hpp with std::vector buffers and memcpy in place of the device copies.  Meant
// to be compiled with -fsanitize=address,undefined (tests/test_pfrt_store_host.py does): an offset or a size that is wrong is a
// heap overflow the sanitizer reports, and a wrong slot shows in the read-back below.  Exit status 0 = all checks passed.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pfrt_store.hpp"

using hipdrt::PfrtStoreLayout;

struct Store {
    PfrtStoreLayout L;
    int max_steps = 0, steps = 0;
    std::vector<double> x, s, rho, rss, slw;
    std::vector<int> status;
    void begin(int cap, int n, int max) {
        L = {(size_t)cap, (size_t)n};
        steps = 0;
        if (max <= max_steps) return;
        // exactly the sizes hipdrt_plan_pfrt_begin allocates: one element too few anywhere is an overflow below
        x.assign(L.x_elems(max), -1.0); s.assign(L.s_elems(max), -1.0); rho.assign(L.rho_elems(max), -1.0);
        rss.assign(L.scalar_elems(max), -1.0); slw.assign(L.scalar_elems(max), -1.0); status.assign(L.scalar_elems(max), -1);
        max_steps = max;
    }
    // the copies of hipdrt_plan_pfrt_record for B staged spectra
    bool record(int B, const double* lx, const double* ls, const double* lrho, const double* lrss, const double* lslw, const int* lst) {
        if (steps >= max_steps) return false;
        const size_t n = L.n, D = sizeof(double);
        std::memcpy(x.data() + L.x(steps), lx, B * n * D);
        std::memcpy(s.data() + L.s(steps), ls, B * 3 * n * D);
        std::memcpy(rho.data() + L.rho(steps), lrho, B * 3 * D);
        std::memcpy(rss.data() + L.scalar(steps), lrss, B * D);
        std::memcpy(slw.data() + L.scalar(steps), lslw, B * D);
        std::memcpy(status.data() + L.scalar(steps), lst, B * sizeof(int));
        ++steps;
        return true;
    }
};

static double tag(int step, int b, int k) { return 1e6 * step + 1e3 * b + k; }

static int run(int cap, int n, int max_steps, int B) {
    Store st;
    st.begin(cap, n, max_steps);
    std::vector<double> lx((size_t)B * n), ls((size_t)B * 3 * n), lrho((size_t)B * 3), lrss(B), lslw(B);
    std::vector<int> lst(B);
    for (int step = 0; step < max_steps; ++step) {
        for (int b = 0; b < B; ++b) {
            for (int k = 0; k < n; ++k) lx[(size_t)b * n + k] = tag(step, b, k);
            for (int k = 0; k < 3 * n; ++k) ls[(size_t)b * 3 * n + k] = tag(step, b, k) + 0.5;
            for (int k = 0; k < 3; ++k) lrho[(size_t)b * 3 + k] = tag(step, b, k) + 0.25;
            lrss[b] = tag(step, b, 0) + 0.125; lslw[b] = tag(step, b, 0) + 0.0625; lst[b] = step * 100 + b;
        }
        if (!st.record(B, lx.data(), ls.data(), lrho.data(), lrss.data(), lslw.data(), lst.data())) return 1;
    }
    if (st.record(B, lx.data(), ls.data(), lrho.data(), lrss.data(), lslw.data(), lst.data())) return 2;      // a full store refuses
    // the step loop of hipdrt_plan_predict_pfrt reads spectrum b of step i at these offsets; rows past B stay untouched
    for (int step = 0; step < max_steps; ++step)
        for (int b = 0; b < cap; ++b) {
            const bool live = b < B;
            for (int k = 0; k < n; ++k)
                if (st.x[st.L.x(step) + (size_t)b * n + k] != (live ? tag(step, b, k) : -1.0)) return 3;
            for (int k = 0; k < 3 * n; ++k)
                if (st.s[st.L.s(step) + (size_t)b * 3 * n + k] != (live ? tag(step, b, k) + 0.5 : -1.0)) return 4;
            for (int k = 0; k < 3; ++k)
                if (st.rho[st.L.rho(step) + (size_t)b * 3 + k] != (live ? tag(step, b, k) + 0.25 : -1.0)) return 5;
            if (st.rss[st.L.scalar(step) + b] != (live ? tag(step, b, 0) + 0.125 : -1.0)) return 6;
            if (st.slw[st.L.scalar(step) + b] != (live ? tag(step, b, 0) + 0.0625 : -1.0)) return 7;
            if (st.status[st.L.scalar(step) + b] != (live ? step * 100 + b : -1)) return 8;
        }
    // the budget a caller is given covers what the store holds (dop_rho included)
    const size_t held = (st.x.size() + st.s.size() + 2 * st.rho.size() + st.rss.size() + st.slw.size()) * sizeof(double) +
                        st.status.size() * sizeof(int);
    if ((long long)held != hipdrt::pfrt_store_bytes_per_spectrum(n, max_steps) * cap) return 9;
    // begin again with fewer steps keeps the buffers and empties the store; more steps grows them
    st.begin(cap, n, max_steps - 1 > 0 ? max_steps - 1 : 1);
    if (st.steps != 0 || st.max_steps != max_steps) return 10;
    st.begin(cap, n, max_steps + 3);
    if (st.max_steps != max_steps + 3 || st.x.size() != st.L.x_elems(max_steps + 3)) return 11;
    return 0;
}

int main() {
    const int shapes[][4] = {{1, 1, 1, 1}, {5, 7, 4, 3}, {5, 7, 4, 5}, {37, 93, 11, 37}, {1024, 514, 11, 1000}};
    for (const auto& sh : shapes) {
        const int rc = run(sh[0], sh[1], sh[2], sh[3]);
        if (rc) { std::printf("capacity %d n %d steps %d B %d: check %d failed\n", sh[0], sh[1], sh[2], sh[3], rc); return rc; }
    }
    if (hipdrt::pfrt_store_bytes_per_spectrum(514, 11) != 11LL * ((4 * 514 + 8) * 8 + 4)) return 20;
    std::printf("pfrt store bookkeeping ok\n");
    return 0;
}
