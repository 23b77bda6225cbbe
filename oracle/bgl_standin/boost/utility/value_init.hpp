// boost/utility/value_init.hpp -- a stand-in, NOT Boost (see ../graph/adjacency_list.hpp).
// boost::initialized_value: converts to a value-initialized object of any type.
#ifndef BGL_STANDIN_VALUE_INIT_HPP
#define BGL_STANDIN_VALUE_INIT_HPP

namespace boost {

struct initialized_value_t {
    template <class T>
    operator T() const { return T(); }
};

const initialized_value_t initialized_value = {};

}  // namespace boost

#endif
