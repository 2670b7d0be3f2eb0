// csrc/hzb_plan.cpp without a device: the chains the launch loop produced before the planner was split out of it
// (tests/golden/hzb_chains.txt), the invariants of hzb_plan_sweep.h over a sweep, hostile inputs, and the layout arithmetic behind
// ur_hzb_layout, ur_hzb_band_pieces and ur_hzb_band_slices.
//
//   g++ -std=c++17 -O1 -g -Wall tests/cpp/test_hzb_plan.cpp unclerenderer_amd/csrc/hzb_plan.cpp
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "hzb_plan_sweep.h"

using hzb_sweep::chain_of;

// A plan in the golden file's words: " | wide FIRST LEVELS depth|mip GRID_X GRID_Y BY0 launch|hold", " | tail FIRST LEVELS launch|hold", " | refused"
static std::string words(const ur::HzbPlan& p)
{
    if (p.status == ur::HzbPlan::not_wide_plus_tail) return " | refused";
    if (p.status != ur::HzbPlan::ok) return " | invalid";
    std::string out;
    for (uint32_t i = 0; i < p.count; ++i) {
        const ur::HzbStep& s = p.steps[i];
        char b[160];
        if (s.kind == ur::HzbStep::wide)
            std::snprintf(b, sizeof b, " | wide %u %u %s %u %u %u %s", s.first, s.levels, s.from_depth ? "depth" : "mip", s.grid_x, s.grid_y, s.by0, s.hold ? "hold" : "launch");
        else
            std::snprintf(b, sizeof b, " | tail %u %u %s", s.first, s.levels, s.hold ? "hold" : "launch");
        out += b;
    }
    return out;
}

// per line: "chain W H mode M done D", "band W H mode M pieces ROW0 ROWS" or "tail W H", then the steps
static int golden(const char* path)
{
    std::ifstream f(path);
    HZB_CHECK(f.good(), "cannot open %s", path);
    int rows = 0, kinds[3] = {0, 0, 0};
    for (std::string line; std::getline(f, line);) {
        if (line.empty() || line[0] == '#') continue;
        const size_t bar = line.find(" |");
        const std::string head = line.substr(0, bar), want = bar == std::string::npos ? "" : line.substr(bar);
        std::istringstream in(head);
        std::string kind, word;
        uint32_t w = 0, h = 0, a = 0, b = 0;
        int mode = 0;
        in >> kind >> w >> h;
        const std::vector<ur_mip_desc> mips = chain_of(w, h);
        ur::HzbPlan p{};
        if (kind == "chain") { in >> word >> mode >> word >> a; p = ur::plan_hzb_chain(w, h, mips.data(), (uint32_t)mips.size(), mode, a != 0); ++kinds[0]; }
        else if (kind == "band") { in >> word >> mode >> word >> a >> b; p = ur::plan_hzb_band(w, h, mips.data(), (uint32_t)mips.size(), mode, a, b); ++kinds[1]; }
        else if (kind == "tail") { p = ur::plan_hzb_tail(mips.data(), (uint32_t)mips.size()); ++kinds[2]; }
        HZB_CHECK(!in.fail() && !mips.empty(), "unreadable row: %s", line.c_str());
        HZB_CHECK(words(p) == want, "%s: planned \"%s\", the loop did \"%s\"", head.c_str(), words(p).c_str(), want.c_str());
        ++rows;
    }
    HZB_CHECK(kinds[0] >= 51 && kinds[1] >= 46 && kinds[2] >= 3, "rows: %d chains, %d bands, %d tails", kinds[0], kinds[1], kinds[2]);
    return rows;
}

// The chains the header comments and the tests name, worked by hand from the rules
static void by_hand()
{
    {   // 64 x 64: mips 32, 16, 8, 4, 2, 1: mips[4] is 2 x 2, so the first step takes five levels and the one-level tail follows: the smallest chain with a tail
        const std::vector<ur_mip_desc> m = chain_of(64, 64);
        const ur::HzbPlan p = ur::plan_hzb_chain(64, 64, m.data(), 6, 1);
        HZB_CHECK(m.size() == 6u && p.count == 2u && p.steps[0].levels == 5u && !p.steps[0].hold && p.steps[1].kind == ur::HzbStep::tail && p.steps[1].levels == 1u && p.steps[1].hold, "64 x 64");
    }
    {   // 16384 x 4200: mips[5] = 256 x 65 = 16640 texels do not fit the tail: four levels, four more from mip 3 (1024 x 262 -> grid 8 x 9 over mip 4's 512 x 131), then six in the tail
        const std::vector<ur_mip_desc> m = chain_of(16384, 4200);
        const ur::HzbPlan p = ur::plan_hzb_chain(16384, 4200, m.data(), (uint32_t)m.size(), 2);
        HZB_CHECK(m.size() == 14u && m[5].width == 256u && m[5].height == 65u && !ur::hzb_chain_is_wide_plus_tail(m.data(), 14), "16384 x 4200: the chain");
        HZB_CHECK(words(p) == " | wide 0 4 depth 128 132 0 launch | wide 4 4 mip 8 9 0 launch | tail 8 6 hold", "16384 x 4200: %s", words(p).c_str());
    }
    {   // 32 x 32: five levels, all in the first step, no tail: nothing to hold in any mode
        const std::vector<ur_mip_desc> m = chain_of(32, 32);
        for (int mode = 0; mode <= 2; ++mode) HZB_CHECK(words(ur::plan_hzb_chain(32, 32, m.data(), 5, mode)) == " | wide 0 5 depth 1 1 0 launch", "32 x 32 mode %d", mode);
    }
}

// ur_hzb_layout's arithmetic against valid_hzb_chain, and a frame's bands against its mips 0-4
static void host_arithmetic()
{
    auto layout = [](uint32_t w, uint32_t h) {
        uint32_t total = 0;
        const std::vector<ur_mip_desc> m = chain_of(w, h, &total);
        const uint32_t n = (uint32_t)m.size();
        HZB_CHECK(n >= 1u && ur::valid_hzb_chain(w, h, m.data(), n) && ur::valid_hzb_chain_below_mip0(m.data(), n), "%u x %u: the layout is not a valid chain", w, h);
        if (n == 0) return;
        HZB_CHECK(m[0].width == (w + 1u) / 2u && m[0].height == (h + 1u) / 2u && m[n - 1].width == 1u && m[n - 1].height == 1u, "%u x %u: first and last level", w, h);
        uint32_t off = 0;
        for (uint32_t k = 0; k < n; ++k) {
            HZB_CHECK(m[k].offset == off && off % 64u == 0u, "%u x %u: level %u at %u", w, h, k, m[k].offset);
            off += (m[k].width * m[k].height + 63u) & ~63u;
            if (k + 1u < n) HZB_CHECK(m[k].width > 1u || m[k].height > 1u, "%u x %u: a 1 x 1 level %u that is not the last", w, h, k);
        }
        HZB_CHECK(off == total, "%u x %u: %u floats, the levels take %u", w, h, total, off);
        // one level fewer, one more (the last repeated), a wrong size: refused where the sizes say so
        std::vector<ur_mip_desc> more = m;
        more.push_back(m[n - 1]);
        HZB_CHECK(n + 1u > UR_MAX_HZB_MIPS || ur::valid_hzb_chain(w, h, more.data(), n + 1u), "%u x %u: 1 x 1 halves to 1 x 1", w, h);
        more[n / 2].height += 1u;
        HZB_CHECK(!ur::valid_hzb_chain(w, h, more.data(), n), "%u x %u: a level one row too tall", w, h);
    };
    for (uint32_t w = 1; w <= 200; ++w)
        for (uint32_t h = 1; h <= 200; ++h) layout(w, h);
    std::mt19937 rng(9);
    for (int k = 0; k < 400; ++k) layout(1u + rng() % 65536u, 1u + rng() % 8192u);
    {
        ur_mip_desc m[UR_MAX_HZB_MIPS];
        uint32_t n = 0;
        HZB_CHECK(ur::hzb_layout(65536, 65536, m, &n) != 0u && n == 16u && ur::hzb_layout(131072, 2, m, &n) == 0u, "the longest chain has 16 levels");
    }
    // the ranks' piece rows tile the wide launch, their slices tile mips 0-4 (each level's rows once, in order)
    const uint32_t frames[][3] = {{3840, 2160, 8}, {1920, 1080, 3}, {1904, 1052, 2}, {7680, 4320, 8}, {3840, 2160, 1}, {3840, 2160, 2}, {3840, 2160, 4}, {129, 67, 1}, {64, 64, 2}};
    for (auto& fr : frames) {
        const uint32_t w = fr[0], h = fr[1], ranks = fr[2];
        const std::vector<ur_mip_desc> m = chain_of(w, h);
        uint32_t next_piece = 0, next[5] = {m[0].offset, m[1].offset, m[2].offset, m[3].offset, m[4].offset};
        for (uint32_t r = 0; r < ranks; ++r) {
            uint32_t row0 = ~0u, rows = ~0u;
            ur::hzb_band_pieces(h, ranks, r, &row0, &rows);
            HZB_CHECK(row0 == next_piece, "%u x %u rank %u of %u: pieces from %u, the rank before ended at %u", w, h, r, ranks, row0, next_piece);
            next_piece = row0 + rows;
            ur_hzb_slice s[5];
            ur::hzb_band_slices(m.data(), row0, rows, s);
            for (uint32_t k = 0; k < 5; ++k) {
                HZB_CHECK(s[k].offset == next[k] && s[k].count % m[k].width == 0u, "%u x %u rank %u level %u: slice at %u (%u floats), expected at %u", w, h, r, k, s[k].offset, s[k].count, next[k]);
                next[k] = s[k].offset + s[k].count;
            }
            const ur::HzbPlan p = ur::plan_hzb_band(w, h, m.data(), (uint32_t)m.size(), 0, row0, rows);
            HZB_CHECK(p.status == ur::HzbPlan::ok && p.count == (rows ? 1u : 0u), "%u x %u rank %u: the band's plan", w, h, r);
        }
        HZB_CHECK(next_piece == (h + 31u) / 32u, "%u x %u: %u piece rows of %u", w, h, next_piece, (h + 31u) / 32u);
        for (uint32_t k = 0; k < 5; ++k) HZB_CHECK(next[k] == m[k].offset + m[k].width * m[k].height, "%u x %u level %u: slices end at %u", w, h, k, next[k]);
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: test_hzb_plan tests/golden/hzb_chains.txt\n"); return 2; }
    const int rows = golden(argv[1]);
    by_hand();
    const long plans = hzb_sweep::sweep();
    const int refused = hzb_sweep::hostile();
    host_arithmetic();
    if (hzb_sweep::g_fail) { std::printf("%d check(s) failed\n", hzb_sweep::g_fail); return 1; }
    std::printf("OK hzb plan: %d recorded chains, %ld swept plans, %d hostile inputs refused\n", rows, plans, refused);
    return 0;
}
