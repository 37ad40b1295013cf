// Scene preparation: everything that turns an rrt_scene_desc into the tables the kernels read, as plain C++17 (no HIP, built by the host compiler).
// Each builder is a free function: a desc or host vectors in, a struct of vectors and scalars out; the driver (device/rrt_impl.hpp upload_scene) uploads
// what comes back. The kernels' tuning constants (treelet sizes, tile-tree sizes, table blocks, the slab pad) are ARGUMENTS here: a tuning variant
// recompiles the fp32 kernel file alone and links these objects unchanged.
//   scene_flatten.cpp   validate_desc, plane_ids, calibrate_aux_margins, scan_materials, flatten_scene
//   sampler_tables.cpp  build_sampler_tables
//   trav_tables.cpp     build_pairs, build_quads, build_tile_trees
//   shadow_lists.cpp    build_shadow_lists
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "errors.hpp"
#include "records.hpp"
#include "rrt.h"

namespace rrtd {

// ---- scene_flatten.cpp ------------------------------------------------------------------------------------------------------------------
// A desc normally comes from rrt_scene_load, but the ABI lets a caller fill one: every index the kernels follow is checked here once
// (a kernel reading past an array can take the GPU down for everybody on the host)
void validate_desc(const rrt_scene_desc* d);

// Plane ids: triangles lying in one plane (unit normals within 1e-6, offsets within 1e-6 of the scene
// diagonal) share an id. Hash on the quantised plane + union-find over neighbouring cells.
std::vector<uint32_t> plane_ids(const std::vector<double>& w, size_t n, const double wb[6]);

// auxiliary-ray margins of the fp32 camera kernels (scene_flatten.cpp has the derivation)
struct AuxMargins { std::vector<float> lim; float delta = 0.0f, pupil = 0.0f; };   // lim: per interface {aperture radius, 16 c_i}, interleaved; 16 c_i = 0: never safe
AuxMargins calibrate_aux_margins(const rrt_scene_desc* d);

// which materials the aggregate really uses (declared-but-unused ones never reach a kernel)
enum class ShadeClass { All, Lambert, Glossy };   // the lobe kinds the USED materials can produce: all of them, Lambert alone, Lambert / Oren-Nayar / microfacet
struct MaterialScan {
  bool has_transmissive = false, has_translucent = false;
  bool area_lights = false;                 // some light is a DiffuseAreaLight
  ShadeClass shade = ShadeClass::All;       // (fp32 only: the f64 mode always shades with the general kernel)
  std::string warning;                      // empty: none
};
MaterialScan scan_materials(const rrt_scene_desc* d, bool fp32);

template <typename R>
inline void affine_rows(const double* m16, R* out12, const char* what) {
  if (m16[12] != 0.0 || m16[13] != 0.0 || m16[14] != 0.0 || m16[15] != 1.0) throw UnsupportedError(std::string(what) + ": projective transform");
  for (int i = 0; i < 12; i++) out12[i] = (R)m16[i];
}

// The desc flattened to the kernels' records: nodes (f64 boxes narrowed outward), primitives in traversal order (world space, kept instances and spheres
// marked), materials, the texture graph, images, lights with their cdf, the lens.
template <typename R>
struct FlatScene {
  std::vector<Node<R>> nodes;
  std::vector<Tri<R>> tris;
  std::vector<TriShade<R>> shades;
  std::vector<SphereDev<R>> spheres;
  std::vector<InstDev<R>> insts;
  std::vector<Material<R>> mats;
  std::vector<TexDev<R>> texs;
  std::vector<ImageDev<R>> imgs;
  std::vector<R> texels;
  std::vector<Light<R>> lights;   // (shadow_tab = 0: the driver fills it in where shadow lists are built)
  std::vector<R> light_cdf;
  double light_func_int = 0.0;    // Distribution1D::func_int of the light cdf
  std::vector<LensElem<R>> lens;
  int tex_depth = 0;              // deepest texture graph some primitive's material evaluates (0 = no textured material in use)
  MaterialScan used;
};
// slab_pad_ulps: fp32 boxes padded outward by that many 2^-24 of the largest coordinate (the FMA slab form of the traversal kernels), 0 = none
template <typename R>
FlatScene<R> flatten_scene(const rrt_scene_desc* d, double slab_pad_ulps);

// ---- sampler_tables.cpp -----------------------------------------------------------------------------------------------------------------
struct HaltonHi { uint32_t rev, pw, bits_lo, bits_hi; };   // one entry of a block table's high part (a uint4 on the device, see HaltonBlk)
struct SamplerTables {
  std::vector<HaltonDim> hdims;   // 1000 dimensions
  std::vector<uint16_t> perms;
  double inv3pow[24];
  uint32_t cam_perm[2];
  double cam_invpow[2][16], cam_tail[2];
  // block tables of the dimensions the integrators draw (SceneDev::hblk / hlo / hhi); blk empty: none
  std::vector<HaltonBlk> blk;
  std::vector<uint32_t> lo;
  std::vector<HaltonHi> hi;
  // block tables of the camera dimensions (SceneDev::cam_lo / cam_hi); has_cam false: none
  bool has_cam = false;
  std::vector<uint32_t> cam_lo;
  std::vector<HaltonHi> cam_hi;
  size_t cam_lo_off[3] = {0, 0, 0}, cam_hi_off[3] = {0, 0, 0};
};
// block_tables: build hblk / cam tables at all (the fp32 mode); n_tab_dims = the dimensions hblk covers; cam_blocks = the low-digit blocks of dimensions 1, 2, 3
SamplerTables build_sampler_tables(const rrt_scene_desc* d, bool block_tables, int n_tab_dims, const uint32_t cam_blocks[3], bool cam_tables);

// ---- trav_tables.cpp (fp32 traversal) ---------------------------------------------------------------------------------------------------
struct PairTables {
  bool ok = false;              // false: this scene keeps the generic kernels (any_list may still hold lists: they are uploaded as before)
  bool mixed = false;           // the tree has kSpecialLeaf leaves (spheres, kept instances)
  uint32_t n_treelet = 0;       // the first n_treelet pair nodes are the BFS top of the tree
  std::vector<uint32_t> any_list;   // TravScene::any_list, 8 words per triangle
  std::vector<PairNode> pairs;
  float root_box[6] = {0, 0, 0, 0, 0, 0};
  uint32_t root_id = 0, n_nodes = 0;
};
// re-pack the linear BVH into pair nodes (see dtraverse_f32.hpp); treelet_nodes = kTreeletNodes
PairTables build_pairs(const std::vector<Node<float>>& nodes, const std::vector<Tri<float>>& tris, int treelet_nodes);

struct QuadTables { std::vector<QuadNode> quads; uint32_t n_qtreelet = 0; };   // quads empty: not built for this scene
// (not for mixed trees: the caller asks only where PairTables::mixed is false); quad_treelet = kQuadTreelet
QuadTables build_quads(const std::vector<Node<float>>& nodes, int quad_treelet);

struct CensusRay { float o[3], d[3]; };
struct Float4 { float x, y, z, w; };
struct TileTreeSizes { uint32_t nodes, tris, local_bytes; };   // kTtNodes, kTtTris, kTtLocalBytes
struct TileTreeTables {
  bool failed = false;             // a worker ran out of memory: no tables
  std::vector<PairNode> shifted;   // local_bytes unused bytes, then the whole tree with its interior child words shifted by local_bytes
  std::vector<PairNode> trees;     // [n_trees + 1][nodes]
  std::vector<Float4> packets;     // [n_trees + 1][tris][3] (tris > 0)
  uint64_t sum_local_tests = 0, sum_tests = 0, sum_nodes = 0, n_with = 0;   // census statistics (RRT_DEBUG)
};
// the census walk and copy selection: rays = the census' camera rays, tree_of = the patch of each
TileTreeTables build_tile_trees(const std::vector<PairNode>& pairs, const std::vector<Tri<float>>& tris, const float root_box[6], const std::vector<CensusRay>& rays,
                                const std::vector<uint32_t>& tree_of, uint32_t n_trees, TileTreeSizes sz);

// ---- shadow_lists.cpp -------------------------------------------------------------------------------------------------------------------
struct ShadowListsHost {
  std::vector<uint32_t> headers, entries;
  std::vector<LeafRec> leaves;
  uint32_t n_tables = 0;
  std::vector<uint32_t> table_of_light;   // per light: table + 1, 0 = none
};
ShadowListsHost build_shadow_lists(const std::vector<Node<float>>& nodes, const std::vector<Tri<float>>& tris, const rrt_scene_desc* d);

}  // namespace rrtd
