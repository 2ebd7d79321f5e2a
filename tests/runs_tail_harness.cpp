// runs_tail_harness.cpp -- TEST-ONLY: the known-runs path of the along-fibre kernel (proxtv_amd/csrc/kernel_along.hpp, RUNS) on the segment
// that holds the fibre's last sample, compiled with g++ next to the models of host_harness.cpp (included: window, ops, walks).
// Built on demand by tests/test_runs_tail_host.py into a temp directory; never linked into libproxtv_amd.so.
#include "host_harness.cpp"

namespace {
constexpr int C = 17, G = 64, H = 16, T = 8, SEG = C * G, ROWS = H + SEG + T;
constexpr unsigned CM = (1u << C) - 1u;

// the window of one segment as the kernel stages it: zone rows before sample 0 are copies of sample 0, rows past the last sample copies
// of the last sample
HostWin stage(const double *y, int len, int seg_s) {
    HostWin win;
    win.lo = seg_s - H;
    win.hi = std::min(len, seg_s + SEG + T);
    for (int i = 0; i < ROWS; i++) win.yy.push_back(y[std::min(std::max(win.lo + i, 0), len - 1)]);
    win.yy.push_back(1e300);
    win.yy.push_back(1e300);
    win.writes.assign(win.yy.size(), 0);
    return win;
}

// every lane walks its chunk speculatively and the links are examined (sweep_along_kernel without RUNS; tests/along_tail_harness.cpp)
bool speculative_records(const HostWin &win, const double *y, double lam, int len, int seg_s, int seg_e, ChunkRec *recs, bool *bad) {
    HostFar far{y, nullptr};
    bool certain[G];
    bool clean = true;
    for (int l = 0; l < G; l++) {
        const int cs = seg_s + l * C, ce = std::min(cs + C, len), start = std::max(0, cs - H);
        certain[l] = bad[l] = false;
        if (!(cs < seg_e)) continue;
        ChunkRec &rec = recs[l];
        Walker wk;
        int cat = -1, ctype = 0;
        if (start > 0 && lam > 0.0) cat = certain_bend_before<false, 8>(win, cs, len, lam, ctype);
        if (cat >= 0) {
            certain[l] = true;
            walker_restart_with<false>(wk, cat, ctype, len, lam, win.y(cat), 0.0, 0.0);
            rec.mine = rec.next = rec.last = ((unsigned)cat << 1) | (unsigned)ctype;
        } else {
            walker_start<false>(wk, win, start, lam);
        }
        walk_interior<false>(wk, rec, win, std::min(len - 1, win.hi), cs, ce, lam);
        TailSource<false, false, 48, HostWin, HostFar> tail{win, far, rec, cs, ce, win.hi, len};
        walker_run<false>(wk, tail, len, lam);
        if (rec.failed) rec.next = 0;
        // (the segment's first lane hangs on another wave: the repair kernel's to check, a certain start or none here)
        const bool linked = !(start == 0 || certain[l]) && l > 0;
        bad[l] = rec.failed || (linked && (rec.mine == 0 || rec.mine != recs[l - 1].next));
        if (l == 0 && !(start == 0 || certain[l])) bad[l] = true;   // (not proven inside the wave: no bits to compare against)
        clean = clean && !bad[l];
    }
    return clean;
}

// The four phases of RUNS on the end segment, the lanes emulated one after the other.  Returns true when the segment is solved run by run
// (recs filled for the lanes that own a chunk, the others left empty); false: it falls back, with the reason counted in stats[4 .. 8].
bool runs_records(const HostWin &win, const double *y, double lam, int len, int sg, int seg_s, int seg_e, ChunkRec *recs, int *stats) {
    HostFar far{y, nullptr};
    // (1) edges: the T edges behind the segment do not exist, the two before it do
    EdgeMasks own[G], m[G];
    for (int l = 0; l < G; l++) own[l] = own_edges<C>(win, seg_s + l * C, lam);
    unsigned xk = 0, xp = 0, xn = 0, xb = 0;
    for (int l = 8; l < 10; l++) {
        unsigned k = 0, pp = 0, nn = 0, bb = 0;
        if (sg > 0) one_edge(win.y(seg_s - 11 + l), win.y(seg_s - 10 + l), lam, k, pp, nn, bb);
        xk |= k << l; xp |= pp << l; xn |= nn << l; xb |= bb << l;
    }
    unsigned BE[G], BT[G], WS[G];
    for (int l = 0; l < G; l++) {
        const int cs = seg_s + l * C, fend = len - cs + kEdgeBias;
        EdgeMasks pv = l ? own[l - 1] : EdgeMasks{}, nx = l < G - 1 ? own[l + 1] : EdgeMasks{};
        if (l == G - 1) { nx.K = (xk & 0xffu) << kEdgeBias; nx.P = (xp & 0xffu) << kEdgeBias; nx.N = (xn & 0xffu) << kEdgeBias; nx.B = (xb & 0xffu) << kEdgeBias; }
        if (l == 0)     { pv.K = ((xk >> 8) & 3u) << C; pv.P = ((xp >> 8) & 3u) << C; pv.N = ((xn >> 8) & 3u) << C; pv.B = ((xb >> 8) & 3u) << C; }
        m[l].K = edge_ext<C>(own[l].K, pv.K, nx.K); m[l].P = edge_ext<C>(own[l].P, pv.P, nx.P);
        m[l].N = edge_ext<C>(own[l].N, pv.N, nx.N); m[l].B = edge_ext<C>(own[l].B, pv.B, nx.B);
        const bool free0 = sg == 0 && l == 0;
        if (free0) m[l].K = (m[l].K & ~7u) | 4u;
        free_end_edges(m[l], fend);
        settle_short_runs(m[l], BE[l], BT[l], WS[l]);
        if (free0) {
            BE[l] = (BE[l] & ~8u) | (m[l].K & 8u);
            BT[l] = (BT[l] & ~8u) | (m[l].P & m[l].K & 8u);
            WS[l] = (WS[l] & ~7u) | ((m[l].K & 8u) ? 0u : 4u);
        }
        free_end_settle(m[l], fend, BE[l], BT[l], WS[l]);
    }
    // (2) the list
    std::vector<unsigned> list;
    bool fail = sg > 0 && (m[0].K & 7u) == 0u;
    if (fail) stats[4]++;
    for (int l = 0; l < G; l++) {
        const int fend = len - (seg_s + l * C) + kEdgeBias;
        unsigned dom = WS[l] & ((1u << (C + kEdgeBias)) - 1u);
        if (l > 0) dom &= ~3u;
        while (dom) {
            const int b = __builtin_ctz(dom);
            dom &= dom - 1u;
            const int e = run_end(m[l].K, b);
            if (e < 0) { fail = true; stats[5]++; }
            else list.push_back(RunEntry::make(l, b, e, (int)((m[l].P >> b) & 1u), sg == 0 && l == 0 && b == kEdgeBias, e == fend).word);
        }
    }
    stats[3] = std::max(stats[3], (int)list.size());
    bool go = !fail && list.size() <= 64;
    if (list.size() > 64) stats[6]++;
    // (3) one run per lane, whether or not the lane owns a chunk
    unsigned E[G] = {}, Tt[G] = {}, hang_word = 0;
    int marks = 0;
    if (go) {
        for (unsigned word : list) {
            const RunEntry en{word};
            const int c0 = seg_s + C * en.lane() - kEdgeBias, a = c0 + en.b(), ee = c0 + en.e();
            if (en.free_end() != (ee == len)) marks++;   // (the mark says what the run's end says)
            ChunkRec rr;
            Walker w;
            if (en.free_start()) {
                walker_start<false>(w, win, 0, lam);
            } else {
                walker_restart_with<false>(w, a, en.type(), len, lam, win.y(a), 0.0, 0.0);
                rr.mine = rr.next = rr.last = ((unsigned)a << 1) | (unsigned)en.type();
            }
            walk_interior<false>(w, rr, win, std::min(len - 1, win.hi), a, ee, lam);
            TailSource<false, false, 48, HostWin, HostFar> tail{win, far, rr, a, ee, win.hi, len};
            walker_run<false>(w, tail, len, lam);
            if (!(rr.done && !rr.failed)) { go = false; stats[7]++; break; }
            if (en.free_end() && !((rr.ends >> (len - 1 - a)) & 1u)) marks++;   // (its last piece ends at sample len - 1)
            stats[2]++;
            const int o = en.b() - kEdgeBias;
            if (o >= 0) {
                E[en.lane()] |= rr.ends << o;
                Tt[en.lane()] |= rr.types << o;
            } else {
                E[0] |= rr.ends >> (-o);
                Tt[0] |= rr.types >> (-o);
                const unsigned low = rr.ends & ((1u << (-o)) - 1u);
                if (low) {
                    const int j = 31 - __builtin_clz(low);
                    hang_word = std::max(hang_word, ((unsigned)(en.b() + j + 2) << 1) | ((rr.types >> j) & 1u));
                }
            }
        }
    }
    if (marks) stats[11] += marks;
    // (4) the chunks' records
    if (go) {
        unsigned ends[G], types[G], lcode[G];
        int lastb[G];
        for (int l = 0; l < G; l++) {
            const int cs = seg_s + l * C, uend = len - 1 - cs;
            const bool has = cs < seg_e;
            const unsigned own_rows = !has ? 0u : (uend >= C - 1 ? CM : (2u << uend) - 1u);
            const unsigned e_prev = l ? E[l - 1] : 0u, t_prev = l ? Tt[l - 1] : 0u;
            ends[l] = ((BE[l] >> (kEdgeBias + 1)) | E[l] | (e_prev >> C)) & own_rows;
            types[l] = ((BT[l] >> (kEdgeBias + 1)) | Tt[l] | (t_prev >> C)) & own_rows & ends[l];
            const unsigned bends = (uend >= 0 && uend < C) ? (ends[l] & ~(1u << uend)) : ends[l];
            lastb[l] = bends ? 31 - __builtin_clz(bends) : -1;
            lcode[l] = lastb[l] >= 0 ? ((((unsigned)(cs + lastb[l] + 1)) << 1) | ((types[l] >> lastb[l]) & 1u)) : 0u;
        }
        unsigned hang = 0;
        if (sg > 0) {
            unsigned best = hang_word;
            const unsigned kb = BE[0] & 7u;
            if (kb) {
                const int bi = 31 - __builtin_clz(kb);
                best = std::max(best, ((unsigned)(bi + 1) << 1) | ((BT[0] >> bi) & 1u));
            }
            if (best) hang = (((unsigned)(seg_s + (int)(best >> 1) - 1 - kEdgeBias)) << 1) | (best & 1u);
        }
        for (int l = 0; l < G && go; l++) {
            if (!(seg_s + l * C < seg_e)) continue;   // (lanes past the last chunk keep empty records)
            unsigned mine = hang;
            for (int k = l - 1; k >= 0; k--)
                if (lastb[k] >= 0) { mine = lcode[k]; break; }
            if (mine == 0u && !(sg == 0 && l == 0)) { go = false; stats[8]++; }
            ChunkRec &rec = recs[l];
            rec.ends = ends[l];
            rec.types = types[l];
            rec.mine = mine;
            rec.next = lastb[l] >= 0 ? lcode[l] : mine;
            rec.last = rec.next;
            rec.done = true;
        }
    }
    return go;
}

void rebuild_end_segment(HostWin &win, const ChunkRec *recs, const bool *bad, double lam, int len, int seg_s, int seg_e) {
    PiecePrefix pres[G];
    for (int l = 0; l < G; l++)
        if (seg_s + l * C < seg_e && !recs[l].failed) pres[l] = first_piece_prefix(win, recs[l], seg_s + l * C, std::max(0, seg_s + l * C - H));
    for (int l = 0; l < G; l++) {
        const int cs = seg_s + l * C, ce = std::min(cs + C, len);
        if (!(cs < seg_e)) continue;
        rebuild_owned<Identity, false, C, 1, false, const double *, 0, 3>(win, recs[l], cs, ce, len, std::max(0, cs - H), !bad[l], seg_s, l == G - 1 || ce == len, lam,
                                                                      (const double *)nullptr, &pres[l]);
    }
}
}  // namespace

extern "C" {
// One fibre; the segment that holds its last sample the way the kernel's wave does it (C = 17, H = 16, T = 8; `endseg` as the kernel
// defines it: not interior, seg_s + SEG >= len).  Rows of every other segment, and of an end segment that falls back, come from the exact
// walk of the whole fibre.  stats: [0] end segments solved run by run, [1] fallen back, [2] runs walked, [3] most runs in one segment,
// [4 .. 8] why segments fell back (no bend at the start, a run without end or longer than a lane takes, > 64 runs, a walk that did not
// close, no bend before a chunk), [9] solved segments whose speculative links all hold (their bits were compared), [10] records that
// differ from the speculative walk's there (ends, types, mine, next), [11] free-end marks that disagree with the run they sit on.
// Returns minus the number of rows (or write counts) that differ from the speculative records through the same rebuild, of rows not
// written exactly once, and of rows written by a path that fell back.
int host_runs_tail(const double *y, double lam, int len, double *x, int *stats) {
    for (int k = 0; k < 12; k++) stats[k] = 0;
    {
        HostSource src{y, nullptr, x, -1};
        Walker w;
        walker_start<false>(w, src, 0, lam);
        walker_run<false>(w, src, len, lam);
    }
    const int nseg = (len + SEG - 1) / SEG;
    int diffs = 0;
    for (int sg = 0; sg < nseg; sg++) {
        const int seg_s = sg * SEG, seg_e = std::min(len, seg_s + SEG);
        const bool interior = seg_s + SEG + T <= len - 1;
        const bool endseg = nseg > 1 && !interior && seg_s < len && seg_s + SEG >= len;   // (nseg == 1: the ONESEG instantiation, no runs)
        if (!endseg || !(lam > 0.0)) continue;
        HostWin win = stage(y, len, seg_s);
        ChunkRec runs[G], spec[G];
        bool none[G] = {}, bad[G];
        const bool solved = runs_records(win, y, lam, len, sg, seg_s, seg_e, runs, stats);
        for (int i = 0; i < ROWS; i++)
            if (win.writes[(size_t)i] != 0) diffs++;   // (nothing is written before phase 4 is through)
        if (!solved) {
            stats[1]++;
            continue;
        }
        stats[0]++;
        HostWin a = win, b = win;
        rebuild_end_segment(a, runs, none, lam, len, seg_s, seg_e);
        if (speculative_records(win, y, lam, len, seg_s, seg_e, spec, bad)) {
            stats[9]++;
            rebuild_end_segment(b, spec, bad, lam, len, seg_s, seg_e);
            for (int i = 0; i < ROWS; i++) {
                if (std::memcmp(&a.yy[(size_t)i], &b.yy[(size_t)i], sizeof(double)) != 0) diffs++;
                if (a.writes[(size_t)i] != b.writes[(size_t)i]) diffs++;
            }
            for (int l = 0; l < G; l++) {
                const bool has = seg_s + l * C < seg_e;
                const ChunkRec &r = runs[l], &s = spec[l];
                if (!has) {
                    if (r.ends || r.types || r.mine || r.next || r.done) stats[10]++;
                } else if (r.ends != s.ends || r.types != s.types || r.mine != s.mine || r.next != s.next) {
                    stats[10]++;
                }
            }
        }
        for (int i = 0; i < ROWS; i++) {
            const int k = win.lo + i;
            const int want = (k >= seg_s && k < seg_e) ? 1 : 0;   // (every row of the segment once, none outside it, none past the fibre)
            if (a.writes[(size_t)i] != want) diffs++;
        }
        for (int k = seg_s; k < seg_e; k++) x[k] = a.y(k);
    }
    return -diffs;
}
}
