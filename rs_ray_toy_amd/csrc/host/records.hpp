// Plain records and word formats shared by the kernels (device/dtypes.hpp, device/dtraverse_f32.hpp) and the host code that prepares a scene for
// them (host/scene_prep.hpp). No HIP header is needed here: every definition exists once, for hipcc and for g++ alike.
#pragma once
#include <stdint.h>

namespace rrtd {
// LinearBVHNode bvh.rs:103-109, narrowed: f32 = 32 B (bounds rounded outward from the f64 build), f64 = 64 B.
// Block tables of a sampler dimension's digit loop (fp32 mode): the sample index is split as hi * block + lo, block = base^low_digits;
// lo[lo_off + lo] = the permuted reversal of exactly low_digits digits, hi[hi_off + hi] = {permuted reversal of hi's digits, base^(digits of hi),
// the two words of the f64 inv_base^(all digits) the loop's running product arrives at}. See scrambled_radical_inverse_tab() in dmath.hpp.
struct HaltonBlk {
  uint32_t block;         // 0 = no table for this dimension
  uint32_t shift;         // l - 1 of the division by `block` (div_base())
  uint32_t magic;         // m'
  uint32_t lo_off, hi_off;
  uint32_t pad[3];
};

template <typename R>
struct alignas(sizeof(R) * 8) Node {
  R bmin[3];
  R bmax[3];
  uint32_t offset;   // leaf: first triangle (traversal order); interior: second child
  uint32_t meta;     // n_primitives << 2 | axis
  // f64: 48 + 8 = 56 -> padded to 64 by alignas
};

// One triangle = 3 world-space vertices + 3 words (48 B in f32). Read by the traversal kernels.
template <typename R>
struct alignas(16) Tri {
  R p0[3], p1[3], p2[3];
  uint32_t material;   // index into materials
  uint32_t shade;      // index into TriShade (0xffffffff: no normals / uvs -> defaults)
  uint32_t plane;      // id shared by exactly coplanar triangles (host, see plane_ids()); used by self_prim()
};

// A sphere primitive of the aggregate occupies one Tri slot (so node.offset still indexes one array in traversal
// order): plane == kSphereMark, shade = index into SceneDev::spheres, material as usual.
constexpr uint32_t kSphereMark = 0xfffffffeu;

// A triangle of a NON-RIGID instance (scale / shear) is not flattened either: the reference transforms the ray into the instance's space,
// re-normalises its direction there and copies the object-space t back to the world ray (TransformedPrimitive::intersect
// primitives.rs:115-139, transform.rs:525-537: Q15), which no world-space triangle reproduces. Such a Tri keeps the mesh's raw vertices
// and carries its instance in the material word: kInstFlag | instance index (15 bits) << 16 | material (16 bits). Its plane id is
// computed from the world-space vertices like everybody's (coplanarity is the same in both spaces).
constexpr uint32_t kInstFlag = 0x80000000u;
template <typename R>
struct InstDev {
  R m[12], mi[12];      // primitive_to_world / its inverse, rows 0..2
  uint32_t identity;    // Transform::is_identity (value compare): the interaction is not transformed then
  uint32_t pad[3];
};

// Sphere (shape/sphere.rs:14-49) + the TransformedPrimitive around it (primitives.rs:100-139). Spheres are not
// flattened: the reference's own sequence of ray transforms is replayed, including its quirks (Q15, Q16).
template <typename R>
struct SphereDev {
  R m[12], mi[12];       // the sphere's obj_to_world / world_to_obj (rows 0..2)
  R im[12], imi[12];     // instance primitive_to_world / its inverse
  R radius, z_min, z_max, theta_min, theta_max, phi_max;
  uint32_t has_inst;     // 0: GeometricPrimitive used directly; 1: wrapped in a TransformedPrimitive
  uint32_t inst_identity;  // TransformedPrimitive::intersect skips the interaction transform for the identity
};

// Optional per-triangle shading attributes (meshes with vn / vt), world space.
template <typename R>
struct TriShade {
  R n[3][3];
  R uv[3][2];
  uint32_t has_n, has_uv;  // mesh_has_* of rrt_tri (0,1,2)
};

template <typename R>
struct Material {
  int32_t type, remap_roughness;
  R kd[3], ks[3], kr[3], eta[3], k[3];
  R sigma, roughness, u_roughness, v_roughness;
  R kt[3], reflect[3], transmit[3], index;   // glass / translucent
  int32_t tex[13];       // RRT_P_* slot -> SceneDev::textures index evaluated at every hit, -1 = the constant above
  int32_t has_tex;       // any slot >= 0
  int32_t bump, pad;     // bump_map texture (Material::bump), -1 = none
};

// one node of the texture graph (rrt_texture, include/rrt.h): float textures carry their value in all three channels
template <typename R>
struct TexDev {
  int32_t type, mapping, aa_none, octaves;
  int32_t child[3], image;   // image: index into SceneDev::images (ImageTexture)
  R fallback[3][3];
  R v[4][3];
  R omega;
  R map[4];
  R vs[3], vt[3];
  R w2t[12];             // world_to_texture rows 0..2 (affine; the loader only composes T * R * S)
};

// MIPMap (rrt_image, include/rrt.h): per level the BlockedArray's data vector as the reference's index expression fills it
struct ImageLevelDev { uint32_t u_res, v_res, u_blocks, n; uint32_t offset, pad[3]; };   // offset / n in texels of SceneDev::image_texels
template <typename R>
struct ImageDev {
  int32_t do_trilinear, wrap, n_levels, pad;
  R max_aniso, pad2;
  ImageLevelDev levels[16];
};

template <typename R>
struct Light {
  int32_t type, shape_type;
  R spectrum[3];
  R p_light[3];
  R area;
  // sphere light shape (object space + transform) / triangle light shape (raw mesh vertices, Q13)
  R m[12], mi[12];                 // obj_to_world rows 0..2 (affine), and inverse
  R radius, z_min, z_max, theta_min, theta_max, phi_max;
  R tp[3][3];                      // triangle vertices
  R tn[3][3];                      // triangle vertex normals (if tri_has_n)
  uint32_t tri_has_n;
  R w_light[3], world_radius;      // DistantLight (lights/distant.rs)
  uint32_t shadow_tab;             // fp32: shadow candidate table of this light + 1 (dtraverse_f32.hpp), 0 = none
};

template <typename R>
struct LensElem { R curvature_radius, thickness, eta, aperture_radius; };

struct HaltonDim {   // one entry per sampler dimension >= 2
  uint32_t base;
  uint32_t perm_offset;   // PRIME_SUMS[dim]
  uint64_t magic;         // m' | (l - 1) << 32 of div_base(): exact a / base for every 32-bit a
  double inv;             // 1 / base: a / base for any 32-bit a = (uint32_t)(a * inv) with a +-1 fix-up (div_base())
  double tail;            // inv * perm[0] / (1 - inv): the infinitely many trailing zero digits of the scrambled radical inverse
};

// ---- fp32 traversal: pair nodes, quad nodes and the child words of both (device/dtraverse_f32.hpp has the kernels and the reasoning) ----
// Field order chosen for the packed fp32 VALU forms (v_pk_add_f32 / v_pk_mul_f32 work on aligned register pairs, and a 128-bit load
// lands in four consecutive registers): every 64-bit half of the three box words pairs two plane coordinates with the SAME ray
// constants - (x, y) against (o.x, o.y) / (inv.x, inv.y), (z, z) against o.z / inv.z - so the 24 subtract / multiply operations of the two
// slab tests are 12 packed instructions. The child words are what the traversal stack holds, ready made.
struct alignas(64) PairNode {
  float xy0[4];               // first child (linear index + 1):  bmin.x, bmin.y, bmax.x, bmax.y
  float xy1[4];               // second child:                    bmin.x, bmin.y, bmax.x, bmax.y
  float zz[4];                // first child bmin.z, bmax.z, second child bmin.z, bmax.z
  uint32_t id0, id1;          // child words: interior = byte offset of its PairNode (bit 31 clear); leaf = kLeafBit | kSpecialLeaf? | n_prims << 19 | first triangle
  uint32_t axis;              // split axis (bvh.rs:183-236: dir_is_neg[axis] visits the second child first)
  uint32_t pad;
};
constexpr uint32_t kLeafBit = 0x80000000u;
// Leaf word = kLeafBit | kSpecialLeaf? | n_prims (11 bits) << 19 | first primitive (19 bits). kSpecialLeaf: the leaf holds a primitive that is
// not a world-space triangle - a sphere (Tri::plane == kSphereMark) or a triangle of a kept instance (Tri::material & kInstFlag, tested in
// object space through the instance's own ray transform, primitives.rs:115-139) - and takes the rare path special_leaf_f32(); only the
// MIXED instantiations of the kernels look at the bit (scenes without such primitives never set it).
constexpr uint32_t kSpecialLeaf = 0x40000000u;
constexpr uint32_t kLeafCountMask = 0x7ffu;
// t_max of the pool's shadow rays (spawn_ray_to: 1 - SHADOW_EPSILON with a unit direction, Q9): the any-hit kernels give every pool shadow
// ray this length, and the host's any-hit start lists (build_pairs()) derive their reach from the same constant
constexpr float kShadowTmax = 1.0f - 0.0001f;
// A lane's position in the walk is one child word: an interior node to visit (byte offset of its PairNode, < kIdle), a leaf to test
// (kLeafBit set), or kIdle. The traversal stack holds the same words with the child's entry distance.
constexpr uint32_t kIdle = 0x7fffffffu;
constexpr uint32_t kSkip0 = 1u, kSkip1 = 2u;   // any-hit list entries (TravScene::any_list): low bits of an interior child word
constexpr int kAnyList = 6;                    // flagged entries per list
struct alignas(128) QuadNode {
  float mnx[4], mny[4], mnz[4];   // bmin of the four slots, one axis per 16-byte word
  float mxx[4], mxy[4], mxz[4];   // bmax
  uint32_t id[4];                 // child words (interior: byte offset of its QuadNode); bits 28-29: split axis of N / of its first child / of its second child / -
  uint32_t pad[4];
};
constexpr uint32_t kQuadAxisShift = 28u, kQuadAxisMask = 3u << 28;
constexpr uint32_t kQuadLeafMax = 511u;   // primitives per leaf the stolen bits leave room for
// shadow candidate lists (dtraverse_f32.hpp "Shadow rays towards delta lights by candidate lists")
constexpr uint32_t kShadowListMax = 48u;        // candidates per (light table, triangle); 0xff in the header = no list: walk the tree
struct LeafRec { float bmin[3]; uint32_t word; float bmax[3]; uint32_t pad; };   // a BVH leaf: its (fp32, outward) box and its leaf word
// tile trees: LDS byte address of slot k of a local copy = the child word that names it (dtraverse_f32.hpp k_trace_tiles_f32)
constexpr uint32_t tt_local_addr(uint32_t k) { return 64u * k + 16u * (k >> 2); }
}  // namespace rrtd
