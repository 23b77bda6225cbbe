// fastq.h -- the quality of a consensus base for `--fastq` (pbdagcon, dazcon).
//
// This build's own definition (the reference writes FASTA only; its workflow, src/cpp/pbdagcon_wf.sh:20-22, turns that
// into FASTQ with a constant quality of 9): from the base's support (dagcon_fetch_support, include/dagcon.h) -- the
// weight of its best-path vertex and the depth at its backbone position -- a Laplace-smoothed fraction of the reads at
// the position that do not pass through the consensus vertex,
//     c = max(depth, weight),  x = c - weight + 1,  Q = floor(10 log10((c + 2) / x)),
// computed exactly in integers: Q is the largest q >= 0 with 10^q * x^10 <= (c + 2)^10.  A depth is at most
// DAGCON_MAX_COVERAGE and a weight one more (dagcon.h), so (c + 2)^10 <= 4097^10 < 2^121 fits unsigned __int128, and
// Q <= 36 ('E').
// tests/support_twin.py is its Python twin.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../../include/dagcon.h"

// -1 where 10 (c + 2)^10 would not fit 128 bits (c > 5600; the device never gives more than DAGCON_MAX_COVERAGE + 1)
inline int dg_quality(uint32_t weight, uint32_t depth) {
    const uint32_t c = depth > weight ? depth : weight;
    if (c > 5600u) return -1;
    const uint32_t x = c - weight + 1;
    unsigned __int128 lhs = 1, rhs = 1;
    for (int i = 0; i < 10; i++) { lhs *= x; rhs *= (c + 2); }
    int q = 0;
    while (lhs * 10 <= rhs) { lhs *= 10; q++; }
    return q;
}

// one record: '@' name '\n' seq '\n' "+\n" qualities '\n'.  False when a quality cannot be computed.
inline bool dg_append_fastq(std::string &out, const std::string &name, const char *seq, uint32_t len,
                            const uint16_t *weight, const uint16_t *depth) {
    out += '@'; out += name; out += '\n';
    out.append(seq, len);
    out += "\n+\n";
    for (uint32_t i = 0; i < len; i++) {
        const int q = dg_quality(weight[i], depth[i]);
        if (q < 0) return false;
        out += (char)(33 + q);
    }
    out += '\n';
    return true;
}

// one result record of pbdagcon, ">%s/%d_%d\n%s\n" (main.cpp:141-143), or with fastq '@' for '>' (src/cpp/pbdagcon_wf.sh:20-22),
// then + and the qualities.  False, with a message, when a quality cannot be computed.
inline bool dg_append_result(std::string &out, bool fastq, const std::string &id, long long r0, long long r1, const char *seq,
                             uint32_t len, const uint16_t *weight, const uint16_t *depth) {
    char head[64];
    snprintf(head, sizeof head, "/%lld_%lld", r0, r1);
    if (fastq) {
        if (dg_append_fastq(out, id + head, seq, len, weight, depth)) return true;
        fprintf(stderr, "pbdagcon: target %s: per-base support out of range\n", id.c_str());
        return false;
    }
    out += '>'; out += id; out += head; out += '\n';
    out.append(seq, len);
    out += '\n';
    return true;
}
