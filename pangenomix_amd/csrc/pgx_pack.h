// Several arrays in ONE allocation, the arithmetic only: no HIP here, a plain host compiler builds tests/pack_layout_check.cpp.
// DevPack (pgx_internal.h) binds it to a workspace slot and to the caller's host arrays.
#pragma once
#include <cstddef>

struct PackPart { size_t off = 0, bytes = 0; };     // one array's place in the allocation

// Every part starts at a multiple of 256 bytes; a part of 0 bytes is legal and occupies nothing.
struct PackLayout {
    size_t off = 0;                                 // where the next part starts
    PackPart add(size_t bytes) {
        const PackPart part{off, bytes};
        off += (bytes + 255) & ~(size_t)255;
        return part;
    }
    size_t total() const { return off; }            // the allocation's size
};
