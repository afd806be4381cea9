// Prints what the GEMM launcher would run (autostyle-tts_amd/csrc/gemm_plan.h: no HIP) for every shape line of a file, as
// "<shape> -> <plan>" ("gemm": one call; "ring": a plain fp16 GEMM under every ring switch; "skinny": an m <= 32 GEMM under every
// combination of its extras; "rows": gemm_rows).  Whatever follows " ->" on an input line is ignored, so the recorded file
// tests/golden/gemm_plan.txt is its own input.  Host-only: built with -fsanitize=address,undefined and run directly by
// tests/test_gemm_plan_cpu.py, which compares the output with that file.  With a second argument N it also times N rounds over the
// list and reports plans per second on stderr (information, never a pass / fail number).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../autostyle-tts_amd/csrc/gemm_plan.h"

using astts::GemmPlan;
using astts::GemmShape;
using astts::RingTile;

namespace {

const char* tile_name(RingTile t) {
    switch (t) {
        case RingTile::T128x128_S2: return "128x128";
        case RingTile::T128x64_S2: return "128x64";
        case RingTile::T64x64_S4: return "64x64";
        case RingTile::T256x256_1B: return "256x256-1barrier";
        case RingTile::T256x256_8P: return "256x256-8phase";
    }
    return "?";
}

std::string describe(const GemmShape& s, const GemmPlan& p) {
    char buf[128];
    switch (p.kind) {
        case ASTTS_GEMM_KIND_SKINNY: {
            if (!p.fits) return "skinny invalid";
            std::snprintf(buf, sizeof buf, "skinny ksplit=%d rows=%d passes=", p.ksplit, p.rows);
            std::string out = buf;
            for (int r0 = 0; r0 < (int)s.m; r0 += p.rows) {
                const int rows = (int)s.m - r0 < p.rows ? (int)s.m - r0 : p.rows;
                const int mt = astts::skinny_mt(rows);
                std::snprintf(buf, sizeof buf, "%s%dxMT%dxXV%d:%zu", r0 ? "," : "", rows, mt, p.xv, astts::skinny_lds_bytes(rows, p.kslice, mt));
                out += buf;
            }
            return out;
        }
        case ASTTS_GEMM_KIND_RING: return std::string("ring ") + tile_name(p.tile);
        case ASTTS_GEMM_KIND_T32: return "T32";
        case ASTTS_GEMM_KIND_T128: return "T128";
        case ASTTS_GEMM_KIND_T128X64: return "T128x64";
        case ASTTS_GEMM_KIND_T64K128: return "T64k128";
        case ASTTS_GEMM_KIND_T64K64: return "T64k64";
    }
    return "?";
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s SHAPES [ROUNDS]\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    std::vector<GemmShape> shapes;
    char line[1024];
    while (std::fgets(line, sizeof line, f)) {
        if (char* p = std::strstr(line, " ->")) *p = 0;
        if (char* p = std::strchr(line, '\n')) *p = 0;
        if (!line[0] || line[0] == '#') {
            std::puts(line);
            continue;
        }
        long long m;
        int n, cin, cin_pad, taps, plain, x16, o16, al, bm, ga, ln, ws, ring, nosplit, k;
        if (std::sscanf(line, "gemm m=%lld n=%d cin=%d cin_pad=%d taps=%d plain=%d x16=%d o16=%d al=%d bm=%d ga=%d ln=%d ws=%d ring=%d nosplit=%d",
                        &m, &n, &cin, &cin_pad, &taps, &plain, &x16, &o16, &al, &bm, &ga, &ln, &ws, &ring, &nosplit) == 15) {
            GemmShape s;
            s.m = m, s.n = n, s.cin = cin, s.cin_pad = cin_pad, s.taps = taps;
            s.plain = plain != 0, s.x_f16 = x16 != 0, s.out_f16 = o16 != 0, s.x_aligned = al != 0;
            s.blockmax = bm != 0, s.gather = ga != 0, s.ln = ln != 0, s.splitk_ws = ws != 0;
            s.ring_mode = ring, s.no_splitk = nosplit != 0;
            shapes.push_back(s);
            std::printf("%s -> %s\n", line, describe(s, astts::gemm_plan(s)).c_str());
        } else if (std::sscanf(line, "ring m=%lld n=%d k=%d bm=%d", &m, &n, &k, &bm) == 4) {
            // a plain fp16 GEMM from an aligned x, fp32 out, under every ring switch -1 .. 5
            std::string out;
            for (int mode = -1; mode <= 5; ++mode) {
                GemmShape s;
                s.m = m, s.n = n, s.cin = s.cin_pad = k, s.x_f16 = true, s.blockmax = bm != 0, s.ring_mode = mode;
                shapes.push_back(s);
                const std::string d = describe(s, astts::gemm_plan(s));
                out += " " + std::to_string(mode) + ":" + (d.rfind("ring ", 0) == 0 ? d.substr(5) : d);
            }
            std::printf("%s ->%s\n", line, out.c_str());
        } else if (std::sscanf(line, "skinny m=%lld n=%d kp=%d", &m, &n, &k) == 3) {
            // a plain fp32 GEMM with m <= 32 under all 16 combinations of (split-K workspace, gather, LayerNorm prologue, ASTTS_NO_SPLITK),
            // in that bit order 0000 .. 1111: a letter per combination, then the plan each letter stands for
            std::vector<std::string> distinct;
            std::string letters;
            for (int v = 0; v < 16; ++v) {
                GemmShape s;
                s.m = m, s.n = n, s.cin = s.cin_pad = k;
                s.splitk_ws = (v & 8) != 0, s.gather = (v & 4) != 0, s.ln = (v & 2) != 0, s.no_splitk = (v & 1) != 0;
                shapes.push_back(s);
                const std::string d = describe(s, astts::gemm_plan(s));
                size_t i = 0;
                while (i < distinct.size() && distinct[i] != d) ++i;
                if (i == distinct.size()) distinct.push_back(d);
                letters += (char)('A' + i);
            }
            std::string out = letters;
            for (size_t i = 0; i < distinct.size(); ++i) out += std::string(" | ") + (char)('A' + i) + ": " + distinct[i];
            std::printf("%s -> %s\n", line, out.c_str());
        } else if (std::sscanf(line, "rows m=%lld n=%d k=%d x16=%d", &m, &n, &k, &x16) == 4) {
            const astts::RowsPlan r = astts::gemm_rows_plan(m, n, k, x16 != 0);
            std::printf("%s -> rows PL=%d RT=%d CT=%d A32=%d\n", line, r.pl, r.rt, r.ct, x16 ? 0 : 1);
        } else {
            std::fprintf(stderr, "gemm_plan: cannot read the line '%s'\n", line);
            return 1;
        }
    }
    std::fclose(f);
    if (argc > 2 && !shapes.empty()) {
        const int rounds = std::atoi(argv[2]);
        long sink = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < rounds; ++r)
            for (const GemmShape& s : shapes) {
                const GemmPlan p = astts::gemm_plan(s);
                sink += p.kind + (int)p.tile + p.rows;
            }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::fprintf(stderr, "gemm_plan: %.1f million plans per second (%zu shapes x %d rounds, checksum %ld)\n",
                     (double)shapes.size() * rounds / sec / 1e6, shapes.size(), rounds, sink);
    }
    return 0;
}
