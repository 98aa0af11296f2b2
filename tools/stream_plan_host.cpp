// The plan of the streamed regressor TSQR (figaroh_plus_amd/csrc/figh_stream_plan.h) on the CPU, for calls given as text:
// no device, no library.  tests/test_streamed_plan_host.py compiles this file and holds its output against the Python
// mirror stream_common.stream_plan.  Build, from the repository root:
//   c++ -std=c++17 -Iinclude -Ifigaroh_plus_amd/csrc tools/stream_plan_host.cpp -o build/stream_plan_host
// (add -fsanitize=address,undefined for a checked run; build/ is git-ignored)
//
// stdin, one call per line, integers separated by blanks:
//   rps ncols nlinks nv njoints is_chain free_flyer mode flags with_tau weighted N chunk_samples chain_capacity
//   nlive [link_pos x nlinks, when nlive >= 0]  n  cols x n
// (nlive, link_pos: what tree_link_positions returns and fills, -1 and nothing where the layout does not apply)
// stdout, one line per call:
//   n nc cs nchunks last padded compact_applies compact nlive ldc chained split nf ncf chain_wgs level0_launches pieces
//   nfirst first x nfirst
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "figh_stream_plan.h"

int main() {
    std::string line;
    int lineno = 0;
    while (std::getline(std::cin, line)) {
        ++lineno;
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        std::istringstream in(line);
        figh::StreamCall c;
        int is_chain = 0, free_flyer = 0, with_tau = 0, weighted = 0;
        long long N = 0, chunk = 0, capacity = 0;
        in >> c.rps >> c.ncols >> c.nlinks >> c.nv >> c.njoints >> is_chain >> free_flyer >> c.mode >> c.flags >> with_tau >>
            weighted >> N >> chunk >> capacity >> c.nlive;
        c.is_chain = is_chain, c.free_flyer = free_flyer, c.with_tau = with_tau, c.weighted = weighted;
        c.N = N, c.chunk_samples = chunk, c.chain_capacity = capacity;
        std::vector<int> link_pos;
        if (in && c.nlive >= 0 && c.nlinks >= 0) {
            link_pos.resize(c.nlinks);
            for (int &p : link_pos) in >> p;
            c.link_pos = link_pos.data();
        }
        in >> c.n;
        std::vector<int32_t> cols(in && c.n > 0 ? c.n : 0);
        for (int32_t &col : cols) in >> col;
        if (!in || c.n < 1 || c.N < 1 || c.rps < 1 || c.ncols < 1) {
            std::fprintf(stderr, "line %d: not a call\n", lineno);
            return 2;
        }
        c.cols = cols.data();
        const figh::StreamPlan p = figh::stream_plan(c);
        std::printf("%d %d %lld %lld %lld %d %d %d %d %lld %d %d %d %d %ld %lld %lld %zu", p.n, p.nc, (long long)p.cs,
                    (long long)p.nchunks, (long long)p.last, (int)p.padded, (int)p.compact_applies, (int)p.compact, p.nlive,
                    (long long)p.ldc, (int)p.chained, (int)p.split, p.nf, p.ncf, p.chain_wgs, (long long)p.level0_launches,
                    (long long)p.pieces, p.first.size());
        for (int32_t f : p.first) std::printf(" %d", f);
        std::printf("\n");
    }
    return 0;
}
