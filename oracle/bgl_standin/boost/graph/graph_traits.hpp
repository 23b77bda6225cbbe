// boost/graph/graph_traits.hpp -- a stand-in, NOT the Boost Graph Library (see adjacency_list.hpp in this folder).
#ifndef BGL_STANDIN_GRAPH_TRAITS_HPP
#define BGL_STANDIN_GRAPH_TRAITS_HPP

namespace boost {

template <class G>
struct graph_traits {
    typedef typename G::vertex_descriptor vertex_descriptor;
    typedef typename G::edge_descriptor edge_descriptor;
    typedef typename G::vertex_iterator vertex_iterator;
    typedef typename G::edge_iterator edge_iterator;
    typedef typename G::out_edge_iterator out_edge_iterator;
    typedef typename G::in_edge_iterator in_edge_iterator;
    typedef typename G::vertices_size_type vertices_size_type;
    typedef typename G::edges_size_type edges_size_type;
    typedef typename G::degree_size_type degree_size_type;
};

}  // namespace boost

#endif
