// sdm_hog_plan.hip -- the launch plan of the lane-packed HOG kernel (HogPlanDev / HogPlanHost, sdm_kernels.h; walked by
// sdm_hog_packed.hip::hog_packed_kernel), built on the host.  No device code and no HIP call: it is a .hip file only so that
// the Makefile's one pattern rule builds it.
#include "sdm_kernels.h"
#include <string.h>
#include <vector>

namespace {
struct PlanLane { int slot, col, active, seg; };
// greedy packing of `npatch` patches of S columns into passes of 64 lanes (see HogPlanDev)
int plan_pack_cut(int S, int npatch, std::vector<std::vector<PlanLane>>& passes, bool allow_cut)
{
    passes.clear();
    std::vector<PlanLane> cur;
    int segs = 0;
    auto flush = [&]() { if (!cur.empty()) passes.push_back(cur); cur.clear(); segs = 0; };
    for (int p = 0; p < npatch; ++p) {
        int c = 0;
        bool continued = false;
        for (;;) {
            const int free_l = 64 - (int)cur.size(), need = S - c;
            if (segs == SDM_PLAN_MAX_SEG || free_l == 0) { flush(); continue; }
            if (need <= free_l) {
                for (int col = c; col < S; ++col)
                    cur.push_back({p, col, (col >= 1 && col <= S - 2 && !(continued && col == c)) ? 1 : 0, segs});
                ++segs;
                break;
            }
            if (free_l >= 3 && allow_cut) {
                // cut: the last placed column is only the right neighbour of the one before it; the next pass starts one
                // column earlier, which there is only the left neighbour
                const int e = c + free_l - 1;
                for (int col = c; col <= e; ++col)
                    cur.push_back({p, col, (col >= 1 && col <= S - 2 && col != e && !(continued && col == c)) ? 1 : 0, segs});
                c = e - 1;
                continued = true;
                flush();
                continue;
            }
            flush();      // fewer than 3 free lanes: no column could contribute
        }
    }
    flush();
    return (int)passes.size();
}
// ... with cuts only if they save a pass (a cut patch's raw cells arrive in two parts, which the descriptor kernel adds)
int plan_pack(int S, int npatch, std::vector<std::vector<PlanLane>>& passes)
{
    std::vector<std::vector<PlanLane>> whole;
    const int pw = plan_pack_cut(S, npatch, whole, false), pc = plan_pack_cut(S, npatch, passes, true);
    if (pw <= pc) { passes.swap(whole); return pw; }
    return pc;
}
// Which cell columns of a cut patch each of its two passes has to move (HogPlanDev: cut word, lane_tab bit 24), read from the
// finished fold tables themselves -- wb and wb16, what the kernels multiply by -- not from the packing: a pixel column feeds its two
// nearest cell columns only, so the pass left of a cut folds exact +0 into the cell columns right of the overlap and the pass
// right of it into those left of it.  jA = the last cell column with a non-zero weight in the pass that holds the patch's
// column 0 (part 0), jB = the first one with a non-zero weight in the other pass (part 1); an uncut patch keeps all C columns.
// A (pass, matrix column) is dropped only where every weight of it, in both tables, is zero (halo lanes have none); false if a
// column of a cut patch would be left without an owner.
bool plan_cut_columns(int C, HogPlanHost& out)
{
    const int NP = out.P + out.Pt, L = (int)out.cut.size();
    auto nonzero = [&](int pt, int n) {
        for (int l = n; l < 64; l += 16) {
            for (int ks = 0; ks < 16; ++ks)
                if (out.wb[((size_t)pt * 64 + l) * 16 + ks] != 0.0f) return true;
            for (int k = 0; k < 32; ++k)
                if (out.wb16[((size_t)pt * 64 + l) * 32 + k] & 0x7fffu) return true;
        }
        return false;
    };
    auto first_landmark = [&](int pt, int slot) { return pt < out.P ? slot : out.n_main * out.G + slot; };
    std::vector<int> jA((size_t)L, -1), jB((size_t)L, C);
    for (int pt = 0; pt < NP; ++pt) {
        const int first_bits = (out.pass_info[(size_t)pt * 4 + 3] >> 24) & 7;
        for (int sg = 0; sg < SDM_PLAN_MAX_SEG; ++sg) {
            const int slot = out.pass_info[(size_t)pt * 4 + sg];
            if (slot < 0) continue;
            int lo = C, hi = -1;
            for (int j = 0; j < C; ++j)
                if (nonzero(pt, sg * C + j)) { if (lo == C) lo = j; hi = j; }
            const int reps = pt < out.P ? out.n_main : 1;      // the passes of the main groups stand for every main group
            for (int g = 0; g < reps; ++g) {
                const int lm = first_landmark(pt, slot) + g * out.G;
                if ((first_bits >> sg) & 1) jA[lm] = hi; else jB[lm] = lo;
            }
        }
    }
    for (int l = 0; l < L; ++l) {
        const bool cut = out.cut[l] != 0;
        if (!cut) { jA[l] = C - 1; jB[l] = C; }
        else if (jA[l] < 0 || jB[l] > C - 1 || jA[l] + 1 < jB[l]) return false;
        out.cut[l] = (cut ? 1 : 0) | (jA[l] << 8) | (jB[l] << 16);
    }
    for (int pt = 0; pt < NP; ++pt) {
        const int first_bits = (out.pass_info[(size_t)pt * 4 + 3] >> 24) & 7;
        unsigned stores = 0;
        for (int sg = 0; sg < SDM_PLAN_MAX_SEG; ++sg) {
            const int slot = out.pass_info[(size_t)pt * 4 + sg];
            if (slot < 0) continue;
            const int w = out.cut[first_landmark(pt, slot)];
            for (int j = 0; j < C; ++j) {
                const bool keep = !(w & 1) || (((first_bits >> sg) & 1) ? j <= ((w >> 8) & 0xff) : j >= ((w >> 16) & 0xff));
                if (!keep && nonzero(pt, sg * C + j)) return false;
                if (keep) stores |= 1u << (sg * C + j);
            }
        }
        for (int x = 0; x < 64; ++x) out.lane_tab[(size_t)pt * 64 + x] |= ((stores >> (x & 15)) & 1u) << 24;
    }
    return true;
}
template <int CELL, int C>
const HogRowConst* compiled_rows()
{
    static constexpr HogRowConstTable<CELL, C> table{};      // constant-evaluated: what the kernel instances of this cell size hold
    return table.r;
}
}  // namespace

const HogRowConst* sdm_hog_compiled_row_consts(int cell, int C)
{
    if (C != 5) return nullptr;
    switch (cell) {      // the cell sizes with specialised instances (sdm_hog_packed.hip: launch_hog_packed)
    case 11: return compiled_rows<11, 5>();
    case 10: return compiled_rows<10, 5>();
    case 8: return compiled_rows<8, 5>();
    case 6: return compiled_rows<6, 5>();
    default: return nullptr;
    }
}

bool sdm_hog_plan_build(const HogLevelDev& lv, int L, HogPlanHost& out)
{
    out = HogPlanHost();
    if (!((lv.O == 4 || lv.O == 9) && lv.C == 5 && lv.cell <= 12 && lv.S >= 4 && lv.S <= 64 && L >= 1)) return false;
    const int S = lv.S;
    for (int d = 0; d < S; ++d) {      // the specialised instances compute the band of a row in integers: must equal the table
        int b; memcpy(&b, &lv.row_tab[d][2], sizeof(int));
        if (b != packed_band_of(d, lv.cell)) return false;
    }
    // ... and the detect instances take the band-slot weights from packed_row_const AS THE COMPILER evaluated it: must be the
    // table's bits, which the host computed at run time (a level that differs gets no packed plan, as with the band above)
    const HogRowConst* compiled = sdm_hog_compiled_row_consts(lv.cell, lv.C);
    for (int d = 0; d < S; ++d) {
        const HogRowConst rc = compiled ? compiled[d] : packed_row_const(d, lv.cell, lv.C);
        if (memcmp(&rc.ws0, &lv.row_tab[d][0], sizeof(float)) || memcmp(&rc.ws1, &lv.row_tab[d][1], sizeof(float))) return false;
    }
    std::vector<std::vector<PlanLane>> tmp;
    // group size: fewest passes per sample, among equals the smaller group (measured and dropped: among equally dense group
    // sizes preferring one with at least two passes per wave, whose per-group set-up is then shared -- measured: the smaller
    // group wins, 1.54 -> 1.50 ms).  Up to 12 patches (round 6; 8 before): nine 55-column patches of the first shipped level share eight
    // passes (495 columns + 2 per cut in 512 lanes) -- 20 passes per RCR-22 face instead of 22, 61 instead of 68 at RCR-68.
    int bestG = 1; long long bestCost = -1;
    for (int G = 1; G <= 12 && G <= L; ++G) {
        const int P = plan_pack(S, G, tmp);
        const int nm = L / G, Gt = L - nm * G;
        const long long cost = (long long)nm * P + (Gt ? plan_pack(S, Gt, tmp) : 0);
        if (bestCost < 0 || cost < bestCost) { bestG = G; bestCost = cost; }
    }
    out.G = bestG; out.n_main = L / bestG; out.Gt = L - out.n_main * bestG;
    std::vector<std::vector<PlanLane>> main_p, tail_p;
    out.P = plan_pack(S, out.G, main_p);
    out.Pt = out.Gt ? plan_pack(S, out.Gt, tail_p) : 0;
    const int NP = out.P + out.Pt;
    out.hist_slots = 2;
    // landmarks whose patch is cut by a pass boundary (its cells are the sum of two partial folds)
    out.cut.assign((size_t)L, 0);
    for (int pt = 0; pt < NP; ++pt) {
        const std::vector<PlanLane>& pl = pt < out.P ? main_p[pt] : tail_p[pt - out.P];
        for (size_t xl = 0; xl < pl.size(); ++xl) {
            const bool starts_here = pl[xl].col == 0;
            if (xl == 0 || pl[xl].slot != pl[xl - 1].slot) {      // first lane of a segment
                if (!starts_here) {                                 // the patch began in the previous pass: cut
                    if (pt < out.P) { for (int g = 0; g < out.n_main; ++g) out.cut[(size_t)g * out.G + pl[xl].slot] = 1; }
                    else out.cut[(size_t)out.n_main * out.G + pl[xl].slot] = 1;
                }
            }
        }
    }
    out.lane_tab.assign((size_t)NP * 64, 0u);
    out.wb.assign((size_t)NP * 64 * 16, 0.0f);
    out.wb16.assign((size_t)NP * 64 * 32, 0);
    out.pass_info.assign((size_t)NP * 4, -1);
    for (int pt = 0; pt < NP; ++pt) {
        const std::vector<PlanLane>& pl = pt < out.P ? main_p[pt] : tail_p[pt - out.P];
        float W[64][16];
        memset(W, 0, sizeof(W));
        int dfirst = 0, dcount = 0;
        for (int x = 0; x < 64; ++x) {
            PlanLane a = x < (int)pl.size() ? pl[x] : PlanLane{pl.back().slot, 0, 0, 3};
            const bool in_use = x < (int)pl.size();
            out.lane_tab[(size_t)pt * 64 + x] = (unsigned)a.slot | ((unsigned)a.col << 8) | ((unsigned)a.active << 16) |
                                               ((unsigned)(in_use ? 1 : 0) << 17) | ((unsigned)a.seg << 20);
            if (!in_use) continue;
            out.pass_info[(size_t)pt * 4 + a.seg] = a.slot;
            if (a.col == S - 1) { if (dcount == 0) dfirst = a.slot; ++dcount; }
            if (a.active) {
                int b; memcpy(&b, &lv.row_tab[a.col][2], sizeof(int));      // cell index floor(hx), hog.c:697-704
                const float w2 = lv.row_tab[a.col][3], w1 = (float)(1.0 - w2);
                if (b >= 0) W[x][a.seg * lv.C + b] = w1;
                if (b + 1 <= lv.C - 1) W[x][a.seg * lv.C + b + 1] = w2;
            }
        }
        // k-step pairs in use, and which segments see their patch for the first time (its column 0 is in this pass)
        int first_bits = 0;
        for (int x = 0; x < (int)pl.size(); ++x)
            if (pl[x].col == 0) first_bits |= 1 << pl[x].seg;
        const int nkp = ((int)pl.size() + 7) / 8;
        out.pass_info[(size_t)pt * 4 + 3] = dfirst | (dcount << 8) | (nkp << 16) | (first_bits << 24);
        int nseg = 0;
        for (int k = 0; k < 3; ++k) nseg += out.pass_info[(size_t)pt * 4 + k] >= 0 ? 1 : 0;
        if (nseg > out.hist_slots) out.hist_slots = nseg;
        for (int l = 0; l < 64; ++l)
            for (int ks = 0; ks < 16; ++ks) out.wb[((size_t)pt * 64 + l) * 16 + ks] = W[4 * ks + (l >> 4)][l & 15];
        // the same weights as two float16 pieces (x 2^10: the second piece of the smallest weight 1 / 24 stays a normal number) in the
        // B-operand layout of v_mfma_f32_16x16x32_f16: lane (li, lq) holds k = 32 kb + 8 lq + 0..7 of column li
        for (int l = 0; l < 64; ++l)
            for (int kb = 0; kb < 2; ++kb)
                for (int j = 0; j < 8; ++j) {
                    const float w = W[32 * kb + 8 * (l >> 4) + j][l & 15] * 1024.0f;
                    const _Float16 h1 = (_Float16)w;
                    const _Float16 h2 = (_Float16)(w - (float)h1);
                    unsigned short b1, b2;
                    memcpy(&b1, &h1, 2); memcpy(&b2, &h2, 2);
                    out.wb16[(((size_t)pt * 64 + l) * 2 + kb) * 16 + j] = b1;
                    out.wb16[(((size_t)pt * 64 + l) * 2 + kb) * 16 + 8 + j] = b2;
                }
    }
    return plan_cut_columns(lv.C, out);
}
