// boost/graph/graphviz.hpp -- a stand-in, NOT the Boost Graph Library (see adjacency_list.hpp in this folder).
// write_graphviz and make_label_writer, for the reference's printGraph(): the dot text BGL documents, a digraph with
// one line per vertex and one per edge, each followed by what its writer prints.
#ifndef BGL_STANDIN_GRAPHVIZ_HPP
#define BGL_STANDIN_GRAPHVIZ_HPP

#include <iostream>

#include <boost/graph/adjacency_list.hpp>

namespace boost {

template <class Map>
struct label_writer {
    Map m;
    template <class Desc>
    void operator()(std::ostream& out, const Desc& d) const { out << "[label=\"" << m[d] << "\"]"; }
};

template <class Map>
label_writer<Map> make_label_writer(Map m) { return label_writer<Map>{m}; }

template <class G, class VertexWriter, class EdgeWriter>
void write_graphviz(std::ostream& out, G& g, VertexWriter vw, EdgeWriter ew) {
    out << "digraph G {\n";
    typename G::vertex_iterator vi, ve;
    for (tie(vi, ve) = vertices(g); vi != ve; ++vi) {
        out << *vi;
        vw(out, *vi);
        out << ";\n";
    }
    typename G::edge_iterator ei, ee;
    for (tie(ei, ee) = edges(g); ei != ee; ++ei) {
        out << source(*ei, g) << "->" << target(*ei, g) << " ";
        ew(out, *ei);
        out << ";\n";
    }
    out << "}\n";
}

}  // namespace boost

#endif
