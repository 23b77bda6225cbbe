// ref_graph_glue.cpp -- extern "C" handles onto the reference's own AlnGraphBoost.cpp.
//
// TEST INFRASTRUCTURE ONLY.  This file is ours; oracle/Makefile compiles it together with the reference's
// src/cpp/AlnGraphBoost.cpp and src/cpp/Alignment.cpp, read in place (never copied, never changed), into
// oracle/_ref/libref_graph.so.  The Boost.Graph headers that AlnGraphBoost.cpp includes are this build's own stand-in
// (oracle/bgl_standin, rules in its adjacency_list.hpp).  The library exists to pin the oracle's restatement of addAln /
// mergeNodes / bestPath / consensus to the real code: tests/test_ref_graph.py.
//
// Access: the merged graph (AlnGraphBoost::_g, _bbMap) is private, and this file has to read it.  The Makefile passes
// -DREF_GRAPH_GLUE_ACCESS on THIS translation unit's compile line alone, and below that define turns `private` into
// `public` for the one #include of AlnGraphBoost.hpp.  Access does not change the class's layout, and the reference's
// own translation units are compiled untouched, without the define.
//
// Stack: mergeInNodes recurses once per merged vertex of a chain (a thousand frames on the `stack` family of
// tests/merge_cases.py), so every call into the reference runs on a thread whose stack is sized here.
#include <pthread.h>

#include <cfloat>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <queue>
#include <string>
#include <vector>

#include <boost/graph/adjacency_list.hpp>
#include <boost/graph/graph_traits.hpp>

#include "Alignment.hpp"
#ifdef REF_GRAPH_GLUE_ACCESS
#define private public
#endif
#include "AlnGraphBoost.hpp"
#ifdef REF_GRAPH_GLUE_ACCESS
#undef private
#endif

namespace {

const size_t STACK_BYTES = size_t(1) << 30;          // reserved, touched only as deep as the recursion goes

template <class F>
struct Call {
    F* f;
    static void* run(void* p) {
        (*static_cast<Call*>(p)->f)();
        return nullptr;
    }
};

// f() on a thread with STACK_BYTES of stack; false when the thread could not be made (f did not run)
template <class F>
bool on_big_stack(F f) {
    pthread_attr_t attr;
    if (pthread_attr_init(&attr) != 0) return false;
    bool ok = pthread_attr_setstacksize(&attr, STACK_BYTES) == 0;
    pthread_t th;
    Call<F> c{&f};
    ok = ok && pthread_create(&th, &attr, &Call<F>::run, &c) == 0;
    pthread_attr_destroy(&attr);
    if (ok) pthread_join(th, nullptr);
    return ok;
}

struct Segment {                                      // oracle.Segment
    int32_t range0, range1;
    char* seq;
};

char* dup(const std::string& s) {
    char* p = static_cast<char*>(std::malloc(s.size() + 1));
    std::memcpy(p, s.c_str(), s.size() + 1);
    return p;
}

size_t segments_out(const std::vector<CnsResult>& seqs, Segment** out) {
    *out = static_cast<Segment*>(std::malloc(sizeof(Segment) * (seqs.size() + 1)));
    for (size_t i = 0; i < seqs.size(); i++) {
        (*out)[i].range0 = seqs[i].range[0];
        (*out)[i].range1 = seqs[i].range[1];
        (*out)[i].seq = dup(seqs[i].seq);
    }
    return seqs.size();
}

struct Opts {                                         // oracle.Opts
    uint32_t min_len, trim;
    int32_t min_weight;
};

// main.cpp:130-137 (or :130 from a backbone string, as the known-answer test constructs it)
AlnGraphBoost* target_graph(uint32_t tlen, const char* backbone, size_t n_alns, const uint32_t* starts,
                            const uint64_t* offs, const uint32_t* lens, const char* qblob, const char* tblob,
                            uint32_t min_len, uint32_t trim) {
    AlnGraphBoost* ag = backbone ? new AlnGraphBoost(std::string(backbone, tlen)) : new AlnGraphBoost(size_t(tlen));
    for (size_t a = 0; a < n_alns; a++) {
        dagcon::Alignment it;
        it.tlen = tlen;
        it.start = starts[a];
        it.qstr.assign(qblob + offs[a], lens[a]);
        it.tstr.assign(tblob + offs[a], lens[a]);
        if (it.qstr.length() < min_len) continue;
        dagcon::Alignment aln = normalizeGaps(it);
        trimAln(aln, int(trim));
        ag->addAln(aln);
    }
    ag->mergeNodes();
    return ag;
}

}  // namespace

extern "C" {

void* rg_new_seq(const char* backbone, size_t len) { return new AlnGraphBoost(std::string(backbone, len)); }

void* rg_new_len(size_t len) { return new AlnGraphBoost(len); }

void rg_free(void* h) { delete static_cast<AlnGraphBoost*>(h); }

void rg_free_ptr(void* p) { std::free(p); }

// addAln on strings that are normalized already (the caller's business, as with og_add_aln)
void rg_add_aln(void* h, uint32_t start, const char* q, const char* t, size_t len) {
    dagcon::Alignment aln;
    aln.start = start;
    aln.qstr.assign(q, len);
    aln.tstr.assign(t, len);
    static_cast<AlnGraphBoost*>(h)->addAln(aln);
}

int rg_merge_nodes(void* h) {
    AlnGraphBoost* ag = static_cast<AlnGraphBoost*>(h);
    return on_big_stack([ag] { ag->mergeNodes(); }) ? 0 : -1;
}

int rg_dangling_nodes(void* h) { return static_cast<AlnGraphBoost*>(h)->danglingNodes() ? 1 : 0; }

// consensus(minWeight): a malloc'd string (rg_free_ptr)
char* rg_consensus_longest(void* h, int min_weight) {
    AlnGraphBoost* ag = static_cast<AlnGraphBoost*>(h);
    std::string s;
    if (!on_big_stack([&] { s = ag->consensus(min_weight); })) return nullptr;
    return dup(s);
}

// consensus(seqs, minWeight, minLen): the number of segments, or -1
long rg_consensus_all(void* h, int min_weight, size_t min_len, Segment** out) {
    AlnGraphBoost* ag = static_cast<AlnGraphBoost*>(h);
    std::vector<CnsResult> seqs;
    if (!on_big_stack([&] { ag->consensus(seqs, min_weight, min_len); })) return -1;
    return long(segments_out(seqs, out));
}

void rg_free_segments(Segment* s, size_t n) {
    for (size_t i = 0; i < n; i++) std::free(s[i].seq);
    std::free(s);
}

// bestPath(): five ints per returned AlnNode (base, weight, coverage, backbone, deleted), malloc'd; the node count or -1
long rg_best_path(void* h, int32_t** out) {
    AlnGraphBoost* ag = static_cast<AlnGraphBoost*>(h);
    std::vector<AlnNode> path;
    if (!on_big_stack([&] { path = ag->bestPath(); })) return -1;
    *out = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (5 * path.size() + 1)));
    for (size_t i = 0; i < path.size(); i++) {
        int32_t* p = *out + 5 * i;
        p[0] = static_cast<unsigned char>(path[i].base);
        p[1] = path[i].weight;
        p[2] = path[i].coverage;
        p[3] = path[i].backbone;
        p[4] = path[i].deleted;
    }
    return long(path.size());
}

size_t rg_num_nodes(void* h) { return *boost::vertices(static_cast<AlnGraphBoost*>(h)->_g).second; }

// The graph as it stands, in the shape of oracle.Graph.adjacency(): per vertex id
//   base, weight, coverage, deleted, n_out, (target, count) x n_out, n_in, (source, count) x n_in
// in list order, as one malloc'd run of ints.  Returns the number of ints.
size_t rg_adjacency(void* h, int32_t** out) {
    AlnGraphBoost* ag = static_cast<AlnGraphBoost*>(h);
    G& g = ag->_g;
    std::vector<int32_t> v;
    VtxIter vi, ve;
    for (boost::tie(vi, ve) = boost::vertices(g); vi != ve; ++vi) {
        const AlnNode& n = g[*vi];
        v.push_back(static_cast<unsigned char>(n.base));
        v.push_back(n.weight);
        v.push_back(n.coverage);
        v.push_back(n.deleted);
        v.push_back(int32_t(boost::out_degree(*vi, g)));
        OutEdgeIter oi, oe;
        for (boost::tie(oi, oe) = boost::out_edges(*vi, g); oi != oe; ++oi) {
            v.push_back(int32_t(boost::target(*oi, g)));
            v.push_back(g[*oi].count);
        }
        v.push_back(int32_t(boost::in_degree(*vi, g)));
        InEdgeIter ii, ie;
        for (boost::tie(ii, ie) = boost::in_edges(*vi, g); ii != ie; ++ii) {
            v.push_back(int32_t(boost::source(*ii, g)));
            v.push_back(g[*ii].count);
        }
    }
    *out = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (v.size() + 1)));
    std::memcpy(*out, v.data(), sizeof(int32_t) * v.size());
    return v.size();
}

// main.cpp:130-137 for one target from the batch layout of og_consensus_target_blob: the merged graph's handle
// (rg_free), or NULL.  The input must conform (the oracle's aln_conforms): the reference does not check.
void* rg_target_graph(uint32_t tlen, const char* backbone, size_t n_alns, const uint32_t* starts,
                      const uint64_t* offs, const uint32_t* lens, const char* qblob, const char* tblob,
                      const Opts* opts) {
    AlnGraphBoost* ag = nullptr;
    if (!on_big_stack([&] {
            ag = target_graph(tlen, backbone, n_alns, starts, offs, lens, qblob, tblob, opts->min_len, opts->trim);
        }))
        return nullptr;
    return ag;
}

// main.cpp:128-138 for one target: the segments (rg_free_segments) and their number, or -1
long rg_consensus_target_blob(uint32_t tlen, const char* backbone, size_t n_alns, const uint32_t* starts,
                              const uint64_t* offs, const uint32_t* lens, const char* qblob, const char* tblob,
                              const Opts* opts, Segment** segs) {
    std::vector<CnsResult> seqs;
    if (!on_big_stack([&] {
            AlnGraphBoost* ag =
                target_graph(tlen, backbone, n_alns, starts, offs, lens, qblob, tblob, opts->min_len, opts->trim);
            ag->consensus(seqs, opts->min_weight, opts->min_len);
            delete ag;
        }))
        return -1;
    return long(segments_out(seqs, segs));
}

}  // extern "C"
