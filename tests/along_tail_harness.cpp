// along_tail_harness.cpp -- TEST-ONLY: the rebuild forms of the along-fibre kernel (proxtv_amd/csrc/kernel_along.hpp) on the segment that
// holds the fibre's last sample, compiled with g++ next to the models of host_harness.cpp (included: window, ops, walks).
// Built on demand by tests/test_along_tail_host.py into a temp directory; never linked into libproxtv_amd.so.
#include "host_harness.cpp"

namespace {
// One fibre, segment by segment, as a wave of the plain 64-lane instantiation sees it (C = 17, H = 16, T = 8): the window is staged the
// way the kernel stages it (zone rows before sample 0: copies of sample 0; rows past the last sample: copies of the last sample), every
// lane walks its chunk speculatively, links are examined, and the segment is rebuilt twice from the same records: once with the general
// form in every lane, once with the form the kernel picks -- FULL = 2 on interior segments, FULL = 3 (a row count per lane) on the
// segment with the fibre's last sample, the general form elsewhere.  The two windows must agree bit for bit, row writes included.
template <class F>
int tail_rebuild_fibre(const double *y, double lam, int len, double *x, int *stats) {
    constexpr int C = 17, G = 64, H = 16, T = 8, SEG = C * G, ROWS = H + SEG + T;
    for (int k = 0; k < 6; k++) stats[k] = 0;
    {
        HostSource src{y, nullptr, x, -1};
        Walker w;
        walker_start<false>(w, src, 0, lam);
        walker_run<false>(w, src, len, lam);
    }
    const int nseg = (len + SEG - 1) / SEG;
    unsigned carried = 0;
    int diffs = 0;
    for (int sg = 0; sg < nseg; sg++) {
        const int seg_s = sg * SEG, seg_e = std::min(len, seg_s + SEG);
        const bool interior = seg_s + SEG + T <= len - 1;
        const bool endseg = !interior && seg_s < len && seg_s + SEG >= len;
        HostWin win;
        win.lo = seg_s - H;
        win.hi = std::min(len, seg_s + SEG + T);
        for (int i = 0; i < ROWS; i++) win.yy.push_back(y[std::min(std::max(win.lo + i, 0), len - 1)]);
        win.yy.push_back(1e300);
        win.yy.push_back(1e300);
        win.writes.assign(win.yy.size(), 0);
        HostFar far{y, nullptr};
        ChunkRec recs[G];
        bool has[G], certain[G], bad[G];
        int starts[G];
        for (int l = 0; l < G; l++) {
            const int cs = seg_s + l * C, ce = std::min(cs + C, len);
            has[l] = cs < seg_e;
            certain[l] = bad[l] = false;
            starts[l] = std::max(0, cs - H);
            if (!has[l]) continue;
            ChunkRec &rec = recs[l];
            Walker wk;
            int cat = -1, ctype = 0;
            if (starts[l] > 0 && lam > 0.0) cat = certain_bend_before<false, 8>(win, cs, len, lam, ctype);
            if (cat >= 0) {
                certain[l] = true;
                walker_restart_with<false>(wk, cat, ctype, len, lam, win.y(cat), 0.0, 0.0);
                rec.mine = rec.next = rec.last = ((unsigned)cat << 1) | (unsigned)ctype;
            } else {
                walker_start<false>(wk, win, starts[l], lam);
            }
            walk_interior<false>(wk, rec, win, std::min(len - 1, win.hi), cs, ce, lam);
            TailSource<false, false, 48, HostWin, HostFar> tail{win, far, rec, cs, ce, win.hi, len};
            walker_run<false>(wk, tail, len, lam);
            if (rec.failed) rec.next = 0;
        }
        bool clean = true;
        int lastl = 0;
        for (int l = 0; l < G; l++) {
            if (!has[l]) continue;
            lastl = l;
            const bool linked = !(starts[l] == 0 || certain[l]);
            const unsigned prev = l > 0 ? recs[l - 1].next : carried;
            bad[l] = recs[l].failed || (linked && (recs[l].mine == 0 || recs[l].mine != prev));
            clean = clean && !bad[l];
        }
        carried = recs[lastl].next;
        PiecePrefix pres[G];
        for (int l = 0; l < G; l++)
            if (has[l] && !recs[l].failed) pres[l] = first_piece_prefix(win, recs[l], seg_s + l * C, starts[l]);
        HostWin general = win, picked = win;
        for (int l = 0; l < G; l++) {
            if (!has[l]) continue;
            const int cs = seg_s + l * C, ce = std::min(cs + C, len);
            const bool last = l == G - 1 || ce == len;
            rebuild_owned<F, false, C>(general, recs[l], cs, ce, len, starts[l], !bad[l], seg_s, last, lam, (const double *)nullptr, &pres[l]);
            if (interior)
                rebuild_owned<F, false, C, 1, false, const double *, 0, 2>(picked, recs[l], cs, ce, len, starts[l], !bad[l], seg_s, l == G - 1, lam,
                                                                          (const double *)nullptr, &pres[l]);
            else if (endseg)
                rebuild_owned<F, false, C, 1, false, const double *, 0, 3>(picked, recs[l], cs, ce, len, starts[l], !bad[l], seg_s, last, lam,
                                                                          (const double *)nullptr, &pres[l]);
            else
                rebuild_owned<F, false, C>(picked, recs[l], cs, ce, len, starts[l], !bad[l], seg_s, last, lam, (const double *)nullptr, &pres[l]);
            if (endseg && ce - cs < C) stats[2]++;
        }
        for (int i = 0; i < ROWS; i++) {
            if (std::memcmp(&general.yy[(size_t)i], &picked.yy[(size_t)i], sizeof(double)) != 0) diffs++;
            if (general.writes[(size_t)i] != picked.writes[(size_t)i]) diffs++;
            const int k = win.lo + i;
            if ((k < seg_s || k >= seg_e) && picked.writes[(size_t)i] != 0) diffs++;   // (nothing outside the segment is written, rows past the fibre least of all)
        }
        if (endseg) stats[0]++;
        if (!clean) {
            stats[1]++;
            continue;
        }
        if (endseg) stats[3]++;
        for (int k = seg_s; k < seg_e; k++) {
            if (picked.writes[(size_t)(k - win.lo)] != 1) diffs++;
            x[k] = F::USES_Y ? 0.5 * (y[k] - picked.y(k)) : picked.y(k);
        }
    }
    return -diffs;
}
}  // namespace

extern "C" {
// stats: [0] segments with the fibre's last sample, [1] segments with an unproven link (their rows come from the exact walk), [2] partial
// chunks rebuilt with a row count, [3] end segments whose rows were taken from the new form.  Returns minus the number of rows (or write
// counts) on which the two forms differ.
int host_tail_rebuild(const double *y, double lam, int len, int reflect, double *x, int *stats) {
    return reflect ? tail_rebuild_fibre<Reflect>(y, lam, len, x, stats) : tail_rebuild_fibre<Identity>(y, lam, len, x, stats);
}
}
