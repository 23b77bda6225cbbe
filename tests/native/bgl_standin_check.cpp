// bgl_standin_check.cpp -- the container rules of oracle/bgl_standin, asserted one by one on small hand-made graphs.
//
// A stand-alone program (tests/test_ref_graph.py builds and runs it, once plain and once under
// -fsanitize=address,undefined).  The rule numbers are those of the comment at the top of
// oracle/bgl_standin/boost/graph/adjacency_list.hpp.  Exit status 0: every rule holds; otherwise the first line that
// failed is printed and the status is 1.  Built with -DBGL_STANDIN_WRONG=1..4 it must fail: the test asserts that too.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include <boost/format.hpp>
#include <boost/graph/adjacency_list.hpp>
#include <boost/graph/graph_traits.hpp>
#include <boost/graph/graphviz.hpp>
#include <boost/utility/value_init.hpp>

#define CHECK(c) \
    do { \
        if (!(c)) { \
            std::printf("FAILED line %d: %s\n", __LINE__, #c); \
            std::exit(1); \
        } \
    } while (0)

typedef boost::adjacency_list<boost::vecS, boost::vecS, boost::bidirectionalS> Bare;

struct Node {
    char base;
    int weight;
    Bare::edge_descriptor best;             // a descriptor of the graph without properties, as AlnNode has
    Node() : base('N'), weight(0) {}
};

struct Edge {
    int count;
    bool visited;
    Edge() : count(0), visited(false) {}
};

typedef boost::adjacency_list<boost::vecS, boost::vecS, boost::bidirectionalS, Node, Edge> G;
typedef boost::graph_traits<G>::vertex_descriptor V;
typedef boost::graph_traits<G>::edge_descriptor E;
typedef boost::graph_traits<G>::vertex_iterator VI;
typedef boost::graph_traits<G>::edge_iterator EI;
typedef boost::graph_traits<G>::out_edge_iterator OI;
typedef boost::graph_traits<G>::in_edge_iterator II;
typedef boost::property_map<G, boost::vertex_index_t>::type IndexMap;

typedef std::vector<std::pair<V, int> > List;          // (other end, count) in list order

static List outs(V u, G& g) {
    List l;
    OI i, e;
    for (boost::tie(i, e) = boost::out_edges(u, g); i != e; ++i) {
        CHECK(boost::source(*i, g) == u);
        l.push_back(std::make_pair(boost::target(*i, g), g[*i].count));
    }
    CHECK(l.size() == out_degree(u, g));
    return l;
}

static List ins(V v, G& g) {
    List l;
    II i, e;
    for (boost::tie(i, e) = boost::in_edges(v, g); i != e; ++i) {
        CHECK(boost::target(*i, g) == v);
        l.push_back(std::make_pair(boost::source(*i, g), g[*i].count));
    }
    CHECK(l.size() == in_degree(v, g));
    return l;
}

// (source, target, count) of the global list, in edges(g) order
static std::vector<std::vector<int> > all_edges(G& g) {
    std::vector<std::vector<int> > l;
    EI i, e;
    for (boost::tie(i, e) = edges(g); i != e; ++i) {
        std::vector<int> r;
        r.push_back(int(boost::source(*i, g)));
        r.push_back(int(boost::target(*i, g)));
        r.push_back(g[*i].count);
        l.push_back(r);
    }
    return l;
}

static E add(V u, V v, int count, G& g) {
    std::pair<E, bool> p = boost::add_edge(u, v, g);
    CHECK(p.second);                                     // rule 3: always adds
    g[p.first].count = count;
    return p.first;
}

static List L(std::initializer_list<std::pair<V, int> > x) { return List(x); }

int main() {
    // rule 1: descriptors are indices, add_vertex appends; the vertex iterator has prefix and postfix ++
    G g;
    g = G(4);                                            // (move assignment, as AlnGraphBoost's constructors do)
    VI vi, ve;
    boost::tie(vi, ve) = boost::vertices(g);
    V first = *vi++;
    CHECK(first == 0 && *vi == 1);
    ++vi;
    CHECK(*vi == 2);
    size_t n = 0;
    for (boost::tie(vi, ve) = boost::vertices(g); vi != ve; ++vi) CHECK(*vi == n++);
    CHECK(n == 4);
    CHECK(g[0].base == 'N' && g[3].weight == 0);          // bundled properties are default-constructed
    V v4 = boost::add_vertex(g);
    CHECK(v4 == 4);
    IndexMap index = boost::get(boost::vertex_index, g);
    CHECK(index[3] == 3 && index[4] == 4);
    g[v4].base = 'T';
    CHECK(g[4].base == 'T');

    // rules 2, 3, 4: insertion order in the global list and in both per-vertex lists; parallel edges
    E e01 = add(0, 1, 10, g);
    E e02 = add(0, 2, 20, g);
    E e12 = add(1, 2, 30, g);
    E e02b = add(0, 2, 40, g);                           // parallel to e02
    E e32 = add(3, 2, 50, g);
    E e03 = add(0, 3, 60, g);
    CHECK(e02 != e02b && e02 == e02);
    CHECK(outs(0, g) == L({{1, 10}, {2, 20}, {2, 40}, {3, 60}}));
    CHECK(ins(2, g) == L({{0, 20}, {1, 30}, {0, 40}, {3, 50}}));
    CHECK(outs(2, g).empty() && ins(0, g).empty());
    std::vector<std::vector<int> > want = {{0, 1, 10}, {0, 2, 20}, {1, 2, 30}, {0, 2, 40}, {3, 2, 50}, {0, 3, 60}};
    CHECK(all_edges(g) == want);

    // rule 5: edge() is the first match of the out list; a missing edge
    E found;
    bool exists;
    boost::tie(found, exists) = edge(0, 2, g);
    CHECK(exists && found == e02 && g[found].count == 20);
    boost::tie(found, exists) = edge(2, 0, g);
    CHECK(!exists);
    E none = boost::initialized_value;
    CHECK(none == E() && found == none);

    // rule 2: a descriptor and a property pointer survive add_vertex and add_edge (many of both: every vector grows)
    Edge* p01 = &g[e01];
    for (int i = 0; i < 200; i++) {
        V nv = boost::add_vertex(g);
        add(0, nv, 1000 + i, g);
        add(nv, 2, 2000 + i, g);
    }
    CHECK(&g[e01] == p01 && g[e01].count == 10 && g[e12].count == 30 && g[e32].count == 50 && g[e03].count == 60);
    g[e02b].count++;
    CHECK(ins(2, g)[2] == std::make_pair(V(0), 41));
    g[e02b].count--;
    std::map<V, E> kept;                                 // descriptors are default-constructible map values
    kept[7] = e32;
    g[1].best = e12;                                     // and assign to the bare graph's descriptor type
    CHECK(g[kept[7]].count == 50 && g[g[1].best].count == 30);

    // rule 6: clear_vertex in the middle of the other end's lists keeps the order of what stays
    G h(6);
    add(0, 5, 1, h);
    add(1, 5, 2, h);
    add(2, 5, 3, h);
    add(3, 5, 4, h);
    add(4, 5, 5, h);
    add(4, 0, 6, h);
    add(4, 1, 7, h);
    add(4, 2, 8, h);
    add(4, 3, 9, h);
    add(1, 1, 11, h);                                    // a self loop at the vertex that goes
    clear_vertex(1, h);
    CHECK(outs(1, h).empty() && ins(1, h).empty());
    CHECK(ins(5, h) == L({{0, 1}, {2, 3}, {3, 4}, {4, 5}}));
    CHECK(outs(4, h) == L({{5, 5}, {0, 6}, {2, 8}, {3, 9}}));
    want = {{0, 5, 1}, {2, 5, 3}, {3, 5, 4}, {4, 5, 5}, {4, 0, 6}, {4, 2, 8}, {4, 3, 9}};
    CHECK(all_edges(h) == want);
    add(1, 5, 12, h);                                    // a cleared vertex is still a vertex
    CHECK(ins(5, h).back() == std::make_pair(V(1), 12) && outs(1, h) == L({{5, 12}}));
    clear_vertex(1, h);

    // rule 7: remove_vertex lowers every descriptor above it, in the lists and in the global list
    remove_vertex(1, h);
    size_t nv = 0;
    for (boost::tie(vi, ve) = boost::vertices(h); vi != ve; ++vi) nv++;
    CHECK(nv == 5);
    CHECK(ins(4, h) == L({{0, 1}, {1, 3}, {2, 4}, {3, 5}}));
    CHECK(outs(3, h) == L({{4, 5}, {0, 6}, {1, 8}, {2, 9}}));
    CHECK(ins(0, h) == L({{3, 6}}) && ins(1, h) == L({{3, 8}}) && ins(2, h) == L({{3, 9}}));
    want = {{0, 4, 1}, {1, 4, 3}, {2, 4, 4}, {3, 4, 5}, {3, 0, 6}, {3, 1, 8}, {3, 2, 9}};
    CHECK(all_edges(h) == want);
    boost::tie(found, exists) = edge(3, 1, h);
    CHECK(exists && h[found].count == 8);

    // write_graphviz, make_label_writer and get(&T::member, g)
    G w(2);
    w[0].base = 'A';
    w[1].base = 'C';
    add(0, 1, 7, w);
    std::ostringstream dot;
    boost::write_graphviz(dot, w, make_label_writer(get(&Node::base, w)), make_label_writer(get(&Edge::count, w)));
    CHECK(dot.str() == "digraph G {\n0[label=\"A\"];\n1[label=\"C\"];\n0->1 [label=\"7\"];\n}\n");

    std::printf("bgl_standin_check: every rule holds\n");
    return 0;
}
