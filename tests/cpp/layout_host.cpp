// Host check of csrc/svsdf_layout.hpp: every offset and total of the four blob layouts against the index arithmetic the
// host layer carried before the layouts were written once (svsdf_check_sub_sw_collision, svsdf_astar_successors,
// astar_alloc, the Polygon block of svsdf_create), written out literally here.  Prints one line per case; exit code 1 on a mismatch.
#include <cstdio>
#include <initializer_list>

#include "../../implicit-svsdf-planner_amd/csrc/svsdf_layout.hpp"

using namespace svsdf_layout;

static int bad = 0;
static void eq(const char *what, size_t got, size_t want) {
  if (got != want) { std::printf("MISMATCH %s: %zu, expected %zu\n", what, got, want); ++bad; }
}

int main() {
  // sub-swept batch, in doubles: [father 3E | child 3E | kt 64 | offsets E+1 (u64) | pts 2T]
  const size_t kMaxKt = 64;
  for (size_t n_edges : {(size_t)1, (size_t)3, (size_t)1000})
    for (size_t total : {(size_t)1, (size_t)5, (size_t)12345}) {
      const SubswLayout L = subsw_layout(n_edges, total, kMaxKt);
      const size_t need = 6 * n_edges + kMaxKt + (n_edges + 1) + 2 * total;
      eq("subsw father", L.father, 0);
      eq("subsw child", L.child, 8 * (3 * n_edges));
      eq("subsw kt", L.kt, 8 * (6 * n_edges));                              // h + 6 * n_edges | d_child + 3 * n_edges
      eq("subsw offs", L.offs, 8 * (6 * n_edges + kMaxKt));                 // h + 6 * n_edges + kMaxKt | d_kt + kMaxKt
      eq("subsw pts", L.pts, 8 * (6 * n_edges + kMaxKt + n_edges + 1));     // ... + n_edges + 1
      eq("subsw bytes", L.bytes, need * sizeof(double));
      eq("subsw growth", L.bytes / sizeof(double) + L.bytes / sizeof(double) / 2, need + need / 2);
      std::printf("subsw E %zu T %zu: %zu bytes\n", n_edges, total, L.bytes);
    }
  // successor batch, bytes per m parents: [yaw 8m | ij 8m || child yaw 72m | stage 9m]
  for (size_t m : {(size_t)1, (size_t)5000, (size_t)1 << 18}) {
    const size_t kIn = 16, kOut = 81, kSuccParents = (size_t)1 << 18;
    const SuccLayout L = succ_layout(m);
    eq("succ yaw", L.yaw, 0);
    eq("succ ij", L.ij, 8 * m);
    eq("succ child_yaw", L.child_yaw, kIn * m);
    eq("succ stage", L.stage, kIn * m + 72 * m);
    eq("succ in", L.in_bytes(), kIn * m);
    eq("succ out", L.out_bytes(), kOut * m);
    eq("succ bytes", L.bytes, m * (kIn + kOut));
    const size_t want = m < kSuccParents ? m : kSuccParents, grown = want + want / 2 < kSuccParents ? want + want / 2 : kSuccParents;
    eq("succ growth", succ_layout(grown).bytes, grown * (kIn + kOut));
    std::printf("succ m %zu: %zu bytes\n", m, L.bytes);
  }
  // A* blob: head 256 | g f yaw | okey oseq path_yaw | father ocell path_cell | id
  const size_t grids[3][2] = {{1, 1}, {13, 70}, {1024, 1024}};
  for (const auto &xy : grids) {
    const size_t cells = xy[0] * xy[1], cap = cells + 1, head = 256;
    const AstarLayout L = astar_layout(cells);
    const size_t d = head, i4 = head + 8 * (3 * cells + 3 * cap);
    eq("astar st", L.st, 0);
    eq("astar g", L.g, d);
    eq("astar f", L.f, d + 8 * cells);
    eq("astar yaw", L.yaw, d + 8 * (2 * cells));
    eq("astar okey", L.okey, d + 8 * (3 * cells));
    eq("astar oseq", L.oseq, d + 8 * (3 * cells + cap));
    eq("astar path_yaw", L.path_yaw, d + 8 * (3 * cells + 2 * cap));
    eq("astar father", L.father, i4);
    eq("astar ocell", L.ocell, i4 + 4 * cells);
    eq("astar path_cell", L.path_cell, i4 + 4 * (cells + cap));
    eq("astar id", L.id, i4 + 4 * (cells + 2 * cap));
    eq("astar bytes", L.bytes, head + 8 * (3 * cells + 3 * cap) + 4 * (cells + 2 * cap) + cells);
    eq("astar open_cap", L.open_cap, cap);
    std::printf("astar %zu x %zu: %zu bytes\n", xy[0], xy[1], L.bytes);
  }
  // Polygon blob: five offsets on 64 bytes.  Header / edge / record sizes: a round set, and one that is no multiple of anything,
  // so that every align() moves its offset.
  const size_t counts[2][4] = {{4, 1, 1, 0}, {1024, 128 * 128 + 2 * 256 * 256, 256 * 32, 7}};
  const size_t sizes[2][3] = {{216, 48, 16}, {201, 47, 13}};
  for (const auto &s : sizes)
    for (const auto &n : counts) {
      auto align = [](size_t o) { return (o + 63) & ~(size_t)63; };
      const size_t o_edges = align(s[0]);
      const size_t o_cell = align(o_edges + n[0] * s[1]);
      const size_t o_slab = align(o_cell + n[1] * s[2]);
      const size_t o_over = align(o_slab + n[2] * s[2]);
      const size_t total = align(o_over + n[3] * sizeof(unsigned short));
      const PolyLayout L = poly_layout(s[0], s[1], s[2], n[0], n[1], n[2], n[3]);
      eq("poly hdr", L.hdr, 0);
      eq("poly edges", L.edges, o_edges);
      eq("poly cells", L.cells, o_cell);
      eq("poly slabs", L.slabs, o_slab);
      eq("poly over", L.over, o_over);
      eq("poly bytes", L.bytes, total);
      if (n[3] == 0) eq("poly empty over", L.bytes, L.over);   // an empty long-list part adds nothing behind the slabs
      std::printf("poly %zu / %zu / %zu / %zu (sizes %zu %zu %zu): %zu bytes\n", n[0], n[1], n[2], n[3], s[0], s[1], s[2], L.bytes);
    }
  std::printf(bad ? "%d mismatches\n" : "all layouts equal\n", bad);
  return bad ? 1 : 0;
}
