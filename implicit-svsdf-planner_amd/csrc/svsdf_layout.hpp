// svsdf_layout.hpp -- the packed blobs of the host layer around the hot path, each laid out once: byte offsets and total of the
// sub-swept batch, the successor batch, the A* search blob and the Polygon blob.  The allocation size, the
// pinned-side pointers and the device-side pointers (or the AstarDev / PolyAccel header fields) all come from the same
// function.  Plain C++ with no HIP and no kernel header: a host compiler builds it alone (tests/cpp/layout_host.cpp).
#pragma once
#include <cstddef>

namespace svsdf_layout {

// Sequential carver: the next `n` elements of T, at the next offset that is a multiple of `align` bytes.
struct Carver {
  size_t end = 0;   // bytes taken so far
  size_t take_bytes(size_t bytes, size_t align) {
    const size_t o = (end + align - 1) / align * align;
    end = o + bytes;
    return o;
  }
  template <typename T> size_t take(size_t n, size_t align = alignof(T)) { return take_bytes(n * sizeof(T), align); }
};

// base + byte offset, as a T*
template <typename T, typename B> T *at(B *base, size_t off) { return reinterpret_cast<T *>(reinterpret_cast<unsigned char *>(base) + off); }

// svsdf_check_sub_sw_collision, one upload: [father 3E | child 3E | kt max_kt | offsets E+1 (u64) | pts 2T], 8-byte elements
struct SubswLayout { size_t father, child, kt, offs, pts, bytes; };
inline SubswLayout subsw_layout(size_t n_edges, size_t n_pts, size_t max_kt) {
  Carver c;
  SubswLayout l;
  l.father = c.take<double>(3 * n_edges);
  l.child = c.take<double>(3 * n_edges);
  l.kt = c.take<double>(max_kt);
  l.offs = c.take<unsigned long long>(n_edges + 1);
  l.pts = c.take<double>(2 * n_pts);
  l.bytes = c.end;
  return l;
}

// svsdf_astar_successors, m parents: one upload [yaw m (f64) | ij 2m (i32)], one read-back [child yaw 9m (f64) | stage 9m (u8)]
struct SuccLayout {
  size_t yaw, ij, child_yaw, stage, bytes;
  size_t in_bytes() const { return child_yaw; }
  size_t out_bytes() const { return bytes - child_yaw; }
};
inline SuccLayout succ_layout(size_t m) {
  Carver c;
  SuccLayout l;
  l.yaw = c.take<double>(m);
  l.ij = c.take<int>(2 * m);
  l.child_yaw = c.take<double>(9 * m);
  l.stage = c.take<unsigned char>(9 * m);
  l.bytes = c.end;
  return l;
}

// svsdf_astar_search on X * Y = cells: [state (head) | g f yaw | open keys, seqs, path yaws | father, open cells, path cells | id];
// the open set and the path hold cells + 1 entries
constexpr size_t kAstarHead = 256;   // bytes kept for AstarState in front of the arrays
struct AstarLayout { size_t st, g, f, yaw, okey, oseq, path_yaw, father, ocell, path_cell, id, bytes, open_cap; };
inline AstarLayout astar_layout(size_t cells) {
  Carver c;
  AstarLayout l;
  l.open_cap = cells + 1;
  l.st = c.take<unsigned char>(kAstarHead);
  l.g = c.take<double>(cells);
  l.f = c.take<double>(cells);
  l.yaw = c.take<double>(cells);
  l.okey = c.take<double>(l.open_cap);
  l.oseq = c.take<unsigned long long>(l.open_cap);
  l.path_yaw = c.take<double>(l.open_cap);
  l.father = c.take<int>(cells);
  l.ocell = c.take<int>(l.open_cap);
  l.path_cell = c.take<int>(l.open_cap);
  l.id = c.take<signed char>(cells);
  l.bytes = c.end;
  return l;
}

// Polygon, one upload: [PolyAccel | edges | cell records | slab records | long lists (u16)], every part and the total on 64 bytes
struct PolyLayout { size_t hdr, edges, cells, slabs, over, bytes; };
inline PolyLayout poly_layout(size_t hdr_bytes, size_t edge_bytes, size_t rec_bytes, size_t n_edges, size_t n_cells,
                              size_t n_slabs, size_t n_over) {
  Carver c;
  PolyLayout l;
  l.hdr = c.take_bytes(hdr_bytes, 64);
  l.edges = c.take_bytes(n_edges * edge_bytes, 64);
  l.cells = c.take_bytes(n_cells * rec_bytes, 64);
  l.slabs = c.take_bytes(n_slabs * rec_bytes, 64);
  l.over = c.take<unsigned short>(n_over, 64);
  l.bytes = c.take_bytes(0, 64);
  return l;
}

}  // namespace svsdf_layout
