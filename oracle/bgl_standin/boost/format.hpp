// boost/format.hpp -- a stand-in, NOT Boost (see graph/adjacency_list.hpp).  The reference's AlnGraphBoost.cpp includes
// this header and uses nothing of it, so it is empty.
#ifndef BGL_STANDIN_FORMAT_HPP
#define BGL_STANDIN_FORMAT_HPP
#endif
