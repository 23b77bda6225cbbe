// ref_graph_sanitize.cpp -- the reference's AlnGraphBoost.cpp and Alignment.cpp on oracle/bgl_standin, as a stand-alone
// program for -fsanitize=address,undefined.
//
// tests/test_ref_graph.py links this file with the reference's two files, compiled from where they lie, and runs it.
// It walks the reference's own loops over the stand-in's iterators: the RawConsensus known-answer input
// (test/cpp/AlnGraphBoostTest.cpp:11-47), then 24 seeded pileups through normalizeGaps, trimAln, addAln, mergeNodes,
// both consensus calls and danglingNodes, and printGraph (reapNodes: remove_vertex) on the first and the last.  An
// iterator that one of those loops invalidates is a heap-use-after-free here.  Prints one line per pileup (the test
// compares them with the oracle's answers); exit status 0 when the known answer came out.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include <boost/graph/adjacency_list.hpp>
#include <boost/graph/graph_traits.hpp>

#include "Alignment.hpp"
#include "AlnGraphBoost.hpp"

static uint64_t state = 0;

static uint32_t rnd(uint32_t n) {                       // a 64-bit LCG (Knuth's MMIX constants), top bits
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return uint32_t((state >> 33) % n);
}

static char base(const std::string& alphabet) { return alphabet[rnd(uint32_t(alphabet.size()))]; }

// argv: backbone, expected consensus, then (tstr, qstr) per alignment of the known-answer input: the test passes them from
// tests/golden/kat_graph.json
int main(int argc, char** argv) {
    if (argc < 5 || argc % 2 == 0) return 2;
    const char* backbone = argv[1];
    const std::string expected = argv[2];
    std::string got;
    {
        AlnGraphBoost ag{std::string(backbone)};
        for (int i = 3; i + 1 < argc; i += 2) {
            dagcon::Alignment a;
            a.start = 1;
            a.tstr = argv[i];
            a.qstr = argv[i + 1];
            ag.addAln(a);                                // (as they stand: the known-answer test does not normalize)
        }
        ag.mergeNodes();
        got = ag.consensus();
        std::ostringstream dot;                          // printGraph writes to std::cout: keep it out of the answers
        std::streambuf* old = std::cout.rdbuf(dot.rdbuf());
        ag.printGraph();
        std::cout.rdbuf(old);
        const std::string text = dot.str();
        std::printf("kat %s dot_lines %zu\n", got.c_str(), size_t(std::count(text.begin(), text.end(), '\n')));
    }

    const std::string alphabets[3] = {"ACGT", "AC", "A"};
    for (int c = 0; c < 24; c++) {
        state = 1000 + c;
        const std::string& al = alphabets[c % 3];
        uint32_t tlen = 1 + rnd(c % 4 == 3 ? 400 : 60), reads = rnd(12);
        int trim = int(rnd(3)), min_weight = int(rnd(3));
        size_t min_len = rnd(5);
        std::string bb;
        for (uint32_t i = 0; i < tlen; i++) bb += base(al);
        AlnGraphBoost* ag = c % 2 ? new AlnGraphBoost(bb) : new AlnGraphBoost(size_t(tlen));
        std::printf("pileup %d tlen %u trim %d min_weight %d min_len %zu bb %s", c, tlen, trim, min_weight, min_len,
                    c % 2 ? bb.c_str() : "-");
        for (uint32_t r = 0; r < reads; r++) {
            uint32_t span = 1 + rnd(tlen), s0 = rnd(tlen - span + 1);
            if (r % 3 == 0) { span = tlen; s0 = 0; }
            dagcon::Alignment a;
            a.tlen = tlen;
            a.start = s0 + 1;                            // conforming: 1-based, inside the target
            if (rnd(3) == 0) { a.qstr += base(al); a.tstr += '-'; }
            for (uint32_t i = s0; i < s0 + span; i++) {
                uint32_t u = rnd(100);
                if (u < 8) { a.qstr += '-'; a.tstr += bb[i]; }
                else if (u < 14) { a.qstr += base(al); a.tstr += bb[i]; }
                else { a.qstr += bb[i]; a.tstr += bb[i]; }
                while (rnd(100) < 15) { a.qstr += base(al); a.tstr += (rnd(4) == 0 ? '.' : '-'); }
            }
            std::printf(" %u %s %s", a.start, a.qstr.c_str(), a.tstr.c_str());
            if (a.qstr.length() < min_len) continue;
            dagcon::Alignment n = normalizeGaps(a);
            trimAln(n, trim);
            ag->addAln(n);
        }
        ag->mergeNodes();
        std::vector<CnsResult> seqs;
        ag->consensus(seqs, min_weight, min_len);
        std::printf(" => longest [%s] dangling %d segments", ag->consensus(min_weight).c_str(), int(ag->danglingNodes()));
        for (size_t i = 0; i < seqs.size(); i++)
            std::printf(" %d_%d_%s", seqs[i].range[0], seqs[i].range[1], seqs[i].seq.c_str());
        std::printf("\n");
        if (c == 23) {
            std::ostringstream dot;
            std::streambuf* old = std::cout.rdbuf(dot.rdbuf());
            ag->printGraph();
            std::cout.rdbuf(old);
        }
        delete ag;
    }
    return got == expected ? 0 : 1;
}
