// boost/graph/adjacency_list.hpp -- a stand-in, NOT the Boost Graph Library.
//
// TEST INFRASTRUCTURE ONLY.  This header is this project's own, written from BGL's documented interface.  It lets
// the reference's AlnGraphBoost.{hpp,cpp} be compiled where they lie (oracle/Makefile, target `ref`) on an image
// without Boost, so that oracle/dagcon_oracle.c can be held to the reference's own graph code.  It provides what those
// two files name and nothing else: one graph type, adjacency_list<vecS, vecS, bidirectionalS, V, E>, with bundled
// properties.  Nothing of Boost and nothing of the reference is copied here.
//
// The container rules it keeps are BGL's for vecS / vecS / bidirectionalS:
//   1. A vertex descriptor is the vertex's index (std::size_t).  add_vertex appends and returns the new index.
//   2. Edge properties live in ONE global list (std::list) in insertion order; edges(g) walks that list front to back.
//      An edge descriptor is (source, target, address of the property in that list); it stays valid across add_vertex
//      and add_edge, and so does a pointer to the property.
//   3. add_edge(u, v, g) always adds and returns (descriptor, true): parallel edges are allowed.  The new edge goes
//      to the BACK of the global list, of u's out list and of v's in list.
//   4. out_edges(u, g) and in_edges(v, g) walk those per-vertex lists in insertion order.
//   5. edge(u, v, g) returns the FIRST entry of u's out list whose target is v, or (a default descriptor, false).
//   6. clear_vertex(u, g) removes every edge at u: from the global list, from u's two lists, and from the list at the
//      other end, where the entries that stay KEEP their order.
//   7. remove_vertex(u, g) erases the vertex (the caller has cleared it, as BGL requires) and lowers every stored
//      descriptor above u by one: in every per-vertex list and in the global edge list.  Descriptors held by the
//      caller go stale, as in BGL.
//   8. Iterator invalidation is std::vector's, per vertex, as in BGL: an out (in) edge iterator is a pointer into u's
//      out (v's in) vector plus the vertex; add_edge at that vertex, clear_vertex at it or at a neighbour, add_vertex
//      and remove_vertex invalidate it.  Vertex iterators are counters and survive add_vertex.
//   9. A vertex property (g[v]) lives in the vertex vector: a reference to it is invalidated by add_vertex.
//
// BGL_STANDIN_WRONG = 1 .. 4 builds a deliberately wrong container, for tests/test_ref_graph.py alone, which shows
// that its comparison notices: 1 new out-edges go to the front of the out list; 2 new in-edges go to the front of the
// in list; 3 clear_vertex fills the hole at the other end with that list's last entry; 4 edges(g) walks the global
// list backwards.
#ifndef BGL_STANDIN_ADJACENCY_LIST_HPP
#define BGL_STANDIN_ADJACENCY_LIST_HPP

#include <algorithm>
#include <cstddef>
#include <iterator>
#include <list>
#include <tuple>
#include <utility>
#include <vector>

#ifndef BGL_STANDIN_WRONG
#define BGL_STANDIN_WRONG 0
#endif

namespace boost {

struct vecS {};
struct bidirectionalS {};
struct no_property {};
enum vertex_index_t { vertex_index };

using std::tie;                            // boost::tie(a, b) = a pair

namespace standin {

// One type for every adjacency_list, whatever its properties: AlnNode stores the descriptors of a graph without
// properties and assigns those of the graph with them.
struct edge_desc {
    std::size_t m_source, m_target;
    void* m_prop;
    edge_desc() : m_source(0), m_target(0), m_prop(nullptr) {}
    edge_desc(std::size_t s, std::size_t t, void* p) : m_source(s), m_target(t), m_prop(p) {}
    bool operator==(const edge_desc& o) const { return m_prop == o.m_prop; }
    bool operator!=(const edge_desc& o) const { return m_prop != o.m_prop; }
};

struct vertex_iter {
    typedef std::forward_iterator_tag iterator_category;
    typedef std::size_t value_type;
    typedef std::ptrdiff_t difference_type;
    typedef const std::size_t* pointer;
    typedef std::size_t reference;
    std::size_t v;
    vertex_iter() : v(0) {}
    explicit vertex_iter(std::size_t x) : v(x) {}
    std::size_t operator*() const { return v; }
    vertex_iter& operator++() { ++v; return *this; }
    vertex_iter operator++(int) { vertex_iter o(*this); ++v; return o; }
    bool operator==(const vertex_iter& o) const { return v == o.v; }
    bool operator!=(const vertex_iter& o) const { return v != o.v; }
};

struct identity_index_map {
    std::size_t operator[](std::size_t v) const { return v; }
};

}  // namespace standin

template <class OutEdgeListS, class VertexListS, class DirectedS, class VertexProp = no_property,
          class EdgeProp = no_property>
class adjacency_list {
public:
    typedef std::size_t vertex_descriptor;
    typedef standin::edge_desc edge_descriptor;
    typedef standin::vertex_iter vertex_iterator;
    typedef std::size_t vertices_size_type;
    typedef std::size_t edges_size_type;
    typedef std::size_t degree_size_type;

    struct edge_rec {
        std::size_t src, tgt;
        EdgeProp prop;
    };
    typedef std::list<edge_rec> edge_list;
    struct stored {                        // an entry of a vertex's out (in) list: the target (source) and the edge
        std::size_t other;
        typename edge_list::iterator it;
    };
    struct vertex_rec {
        std::vector<stored> out, in;
        VertexProp prop;
    };

    template <bool Out>
    struct incident_iter {                 // rule 8: a pointer into the vertex's vector
        typedef std::forward_iterator_tag iterator_category;
        typedef edge_descriptor value_type;
        typedef std::ptrdiff_t difference_type;
        typedef const edge_descriptor* pointer;
        typedef edge_descriptor reference;
        const stored* p;
        std::size_t at;
        incident_iter() : p(nullptr), at(0) {}
        incident_iter(const stored* q, std::size_t v) : p(q), at(v) {}
        edge_descriptor operator*() const {
            return Out ? edge_descriptor(at, p->other, &p->it->prop) : edge_descriptor(p->other, at, &p->it->prop);
        }
        incident_iter& operator++() { ++p; return *this; }
        incident_iter operator++(int) { incident_iter o(*this); ++p; return o; }
        bool operator==(const incident_iter& o) const { return p == o.p; }
        bool operator!=(const incident_iter& o) const { return p != o.p; }
    };
    typedef incident_iter<true> out_edge_iterator;
    typedef incident_iter<false> in_edge_iterator;

    struct edge_iterator {
        typedef std::forward_iterator_tag iterator_category;
        typedef edge_descriptor value_type;
        typedef std::ptrdiff_t difference_type;
        typedef const edge_descriptor* pointer;
        typedef edge_descriptor reference;
#if BGL_STANDIN_WRONG == 4
        typedef typename edge_list::reverse_iterator base_iter;
#else
        typedef typename edge_list::iterator base_iter;
#endif
        base_iter i;
        edge_iterator() {}
        explicit edge_iterator(base_iter x) : i(x) {}
        edge_descriptor operator*() const { return edge_descriptor(i->src, i->tgt, &i->prop); }
        edge_iterator& operator++() { ++i; return *this; }
        edge_iterator operator++(int) { edge_iterator o(*this); ++i; return o; }
        bool operator==(const edge_iterator& o) const { return i == o.i; }
        bool operator!=(const edge_iterator& o) const { return i != o.i; }
    };

    adjacency_list() {}
    explicit adjacency_list(std::size_t n) : m_vertices(n) {}
    // the per-vertex lists hold iterators into m_edges: a move keeps them valid (std::list), a copy would not
    adjacency_list(adjacency_list&&) = default;
    adjacency_list& operator=(adjacency_list&&) = default;
    adjacency_list(const adjacency_list&) = delete;
    adjacency_list& operator=(const adjacency_list&) = delete;

    VertexProp& operator[](vertex_descriptor v) { return m_vertices[v].prop; }
    const VertexProp& operator[](vertex_descriptor v) const { return m_vertices[v].prop; }
    EdgeProp& operator[](const edge_descriptor& e) { return *static_cast<EdgeProp*>(e.m_prop); }
    const EdgeProp& operator[](const edge_descriptor& e) const { return *static_cast<const EdgeProp*>(e.m_prop); }

    std::vector<vertex_rec> m_vertices;
    edge_list m_edges;
};

#define BGL_STANDIN_TMPL template <class O, class V, class D, class VP, class EP>
#define BGL_STANDIN_G adjacency_list<O, V, D, VP, EP>

BGL_STANDIN_TMPL
typename BGL_STANDIN_G::vertex_descriptor add_vertex(BGL_STANDIN_G& g) {
    g.m_vertices.emplace_back();
    return g.m_vertices.size() - 1;
}

BGL_STANDIN_TMPL
std::pair<typename BGL_STANDIN_G::edge_descriptor, bool> add_edge(std::size_t u, std::size_t v, BGL_STANDIN_G& g) {
    typedef typename BGL_STANDIN_G::stored stored;
    typedef typename BGL_STANDIN_G::edge_rec edge_rec;
    g.m_edges.push_back(edge_rec{u, v, EP()});
    typename BGL_STANDIN_G::edge_list::iterator it = std::prev(g.m_edges.end());
    std::vector<stored>& out = g.m_vertices[u].out;
    std::vector<stored>& in = g.m_vertices[v].in;
#if BGL_STANDIN_WRONG == 1
    out.insert(out.begin(), stored{v, it});
#else
    out.push_back(stored{v, it});
#endif
#if BGL_STANDIN_WRONG == 2
    in.insert(in.begin(), stored{u, it});
#else
    in.push_back(stored{u, it});
#endif
    return std::make_pair(typename BGL_STANDIN_G::edge_descriptor(u, v, &it->prop), true);
}

BGL_STANDIN_TMPL
std::pair<typename BGL_STANDIN_G::vertex_iterator, typename BGL_STANDIN_G::vertex_iterator>
vertices(const BGL_STANDIN_G& g) {
    typedef typename BGL_STANDIN_G::vertex_iterator I;
    return std::make_pair(I(0), I(g.m_vertices.size()));
}

BGL_STANDIN_TMPL
std::pair<typename BGL_STANDIN_G::edge_iterator, typename BGL_STANDIN_G::edge_iterator> edges(BGL_STANDIN_G& g) {
    typedef typename BGL_STANDIN_G::edge_iterator I;
#if BGL_STANDIN_WRONG == 4
    return std::make_pair(I(g.m_edges.rbegin()), I(g.m_edges.rend()));
#else
    return std::make_pair(I(g.m_edges.begin()), I(g.m_edges.end()));
#endif
}

BGL_STANDIN_TMPL
std::pair<typename BGL_STANDIN_G::out_edge_iterator, typename BGL_STANDIN_G::out_edge_iterator>
out_edges(std::size_t u, const BGL_STANDIN_G& g) {
    typedef typename BGL_STANDIN_G::out_edge_iterator I;
    const std::vector<typename BGL_STANDIN_G::stored>& l = g.m_vertices[u].out;
    return std::make_pair(I(l.data(), u), I(l.data() + l.size(), u));
}

BGL_STANDIN_TMPL
std::pair<typename BGL_STANDIN_G::in_edge_iterator, typename BGL_STANDIN_G::in_edge_iterator>
in_edges(std::size_t v, const BGL_STANDIN_G& g) {
    typedef typename BGL_STANDIN_G::in_edge_iterator I;
    const std::vector<typename BGL_STANDIN_G::stored>& l = g.m_vertices[v].in;
    return std::make_pair(I(l.data(), v), I(l.data() + l.size(), v));
}

BGL_STANDIN_TMPL
std::size_t source(const standin::edge_desc& e, const BGL_STANDIN_G&) { return e.m_source; }

BGL_STANDIN_TMPL
std::size_t target(const standin::edge_desc& e, const BGL_STANDIN_G&) { return e.m_target; }

BGL_STANDIN_TMPL
std::size_t out_degree(std::size_t u, const BGL_STANDIN_G& g) { return g.m_vertices[u].out.size(); }

BGL_STANDIN_TMPL
std::size_t in_degree(std::size_t v, const BGL_STANDIN_G& g) { return g.m_vertices[v].in.size(); }

BGL_STANDIN_TMPL
std::pair<typename BGL_STANDIN_G::edge_descriptor, bool> edge(std::size_t u, std::size_t v, const BGL_STANDIN_G& g) {
    typedef typename BGL_STANDIN_G::edge_descriptor E;
    const std::vector<typename BGL_STANDIN_G::stored>& l = g.m_vertices[u].out;
    for (std::size_t i = 0; i < l.size(); i++)
        if (l[i].other == v) return std::make_pair(E(u, v, &l[i].it->prop), true);
    return std::make_pair(E(), false);
}

namespace standin {
// take the entry of edge `it` out of the list at the other end (rule 6)
template <class Stored, class It>
void drop_entry(std::vector<Stored>& l, It it) {
    for (std::size_t i = 0; i < l.size(); i++) {
        if (l[i].it != it) continue;
#if BGL_STANDIN_WRONG == 3
        l[i] = l.back();
        l.pop_back();
#else
        l.erase(l.begin() + i);
#endif
        return;
    }
}
}  // namespace standin

BGL_STANDIN_TMPL
void clear_vertex(std::size_t u, BGL_STANDIN_G& g) {
    typedef typename BGL_STANDIN_G::stored stored;
    std::vector<stored> out;
    out.swap(g.m_vertices[u].out);
    for (std::size_t i = 0; i < out.size(); i++) {       // (a self loop's in entry leaves u's in list here)
        standin::drop_entry(g.m_vertices[out[i].other].in, out[i].it);
        g.m_edges.erase(out[i].it);
    }
    std::vector<stored> in;
    in.swap(g.m_vertices[u].in);
    for (std::size_t i = 0; i < in.size(); i++) {
        standin::drop_entry(g.m_vertices[in[i].other].out, in[i].it);
        g.m_edges.erase(in[i].it);
    }
}

BGL_STANDIN_TMPL
void remove_vertex(std::size_t u, BGL_STANDIN_G& g) {
    g.m_vertices.erase(g.m_vertices.begin() + u);
    for (std::size_t v = 0; v < g.m_vertices.size(); v++) {
        for (auto& s : g.m_vertices[v].out) if (s.other > u) s.other--;
        for (auto& s : g.m_vertices[v].in) if (s.other > u) s.other--;
    }
    for (auto& e : g.m_edges) {
        if (e.src > u) e.src--;
        if (e.tgt > u) e.tgt--;
    }
}

// property_map<G, vertex_index_t>::type and get(vertex_index, g): the identity
template <class G, class Tag>
struct property_map;

template <class G>
struct property_map<G, vertex_index_t> {
    typedef standin::identity_index_map type;
    typedef standin::identity_index_map const_type;
};

BGL_STANDIN_TMPL
standin::identity_index_map get(vertex_index_t, const BGL_STANDIN_G&) { return standin::identity_index_map(); }

// get(&Bundle::member, g): a map from a descriptor to that member of its bundled property
namespace standin {
template <class G, class T, class M>
struct member_map {
    const G* g;
    M T::*m;
    const M& operator[](std::size_t v) const { return ((*g)[v]).*m; }
    const M& operator[](const edge_desc& e) const { return ((*g)[e]).*m; }
};
}  // namespace standin

template <class T, class M, class O, class V, class D, class VP, class EP>
standin::member_map<BGL_STANDIN_G, T, M> get(M T::*m, const BGL_STANDIN_G& g) {
    return standin::member_map<BGL_STANDIN_G, T, M>{&g, m};
}

#undef BGL_STANDIN_TMPL
#undef BGL_STANDIN_G

}  // namespace boost

#endif
