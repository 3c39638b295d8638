// capi.hip — the C-ABI of include/flashsdf.h: the context (ctx.h) and its
// settings, the resident model, point queries and ray casts, profiling. The
// resident cloud is cloud.hip's, the three-launch residual pass (pose -> pass
// -> reduce) pass.hip's, mechanism iterations iterate.hip's, solver loops descend.hip's.
//
// Ownership mirrors the reference: the cloud is held for a whole frame
// (CostFunctor keeps sensed_points by reference, src/gradientdescent.jl:41-47)
// and every evaluation only ships the K poses (what set_configuration! +
// transform_to_root produce in src/Flash.jl:248). No CPU fallback exists: a
// context cannot be created without a HIP device.

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <utility>
#include <vector>

#include "ctx.h"

// the model's device memory and what was derived from the model; the context's
// settings stay
static void free_model(fsdf_ctx* c) {
  c->model = ModelBuffers();
  for (int i = 0; i < kPoseRing; ++i) {
    if (c->rbf_ev[i]) (void)hipEventSynchronize(c->rbf_ev[i]);
    c->h_rbf[i].reset();
  }
  c->rbf_slot = 0;
  c->rbf_ready = false;
  c->posed = PosedBuffers();
  c->rbf32.reset();
  c->pm = fsdf::PosedModel();
  // (the partition tiers are a context setting: they survive a model change)
  const int64_t h4 = c->lm.hpart4_points, h2 = c->lm.hpart2_points;
  c->plan_nc = -1;
  c->prior_ok = c->prior_pass = false;  // seeds name surfaces of the old model
  c->solver_tree_ok = false;  // (its surface list)
  c->last_pass_shape = 0;
  c->lm = fsdf::LocalModel();
  c->lm.hpart4_points = h4;
  c->lm.hpart2_points = h2;
}

extern "C" int fsdf_create(fsdf_ctx** out, const fsdf_opts* opts) {
  if (!out) return FSDF_ERR_ARG;
  *out = nullptr;
  fsdf_ctx* c = new (std::nothrow) fsdf_ctx();
  if (!c) return FSDF_ERR_NOMEM;
  if (opts) {
    c->device = opts->device;
    c->precision = opts->precision ? opts->precision : 64;
    c->sort_points = opts->sort_points;
    c->cull = opts->cull;
  }
  if (c->precision != 64 && c->precision != 32) {
    delete c;
    return FSDF_ERR_ARG;
  }
  int ndev = 0;
  // the prefetch copy stream right after the context stream: HIP hands out its
  // hardware queues round robin by stream creation, so the two land on
  // different queues (on a shared one the copy would serialise with the passes)
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || c->device < 0 || c->device >= ndev ||
      hipSetDevice(c->device) != hipSuccess || c->own_stream.create() != hipSuccess ||
      c->copy_stream.create() != hipSuccess || c->ev_prefetch.create(hipEventDisableTiming) != hipSuccess) {
    delete c;
    return FSDF_ERR_HIP;
  }
  c->stream = c->own_stream;
  *out = c;
  return FSDF_OK;
}

extern "C" int fsdf_destroy(fsdf_ctx* c) {
  if (!c) return FSDF_ERR_ARG;
  (void)hipSetDevice(c->device);  // (before anything is freed: contexts of several devices share a process)
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  delete c;
  return FSDF_OK;
}

extern "C" const char* fsdf_last_error(const fsdf_ctx* c) {
  if (!c) return "null context";
  return c->err.c_str();
}

extern "C" int fsdf_set_stream(fsdf_ctx* c, void* s) {
  if (!c) return FSDF_ERR_ARG;
  c->stream = s == FSDF_HIP_NULL_STREAM ? (hipStream_t)0 : (s ? (hipStream_t)s : c->own_stream);
  return FSDF_OK;
}

extern "C" int fsdf_num_hulls(const fsdf_ctx* c, int32_t* k) {
  if (!c || !k) return FSDF_ERR_ARG;
  *k = c->lm.S;  // surfaces of every kind = poses expected per pass
  return FSDF_OK;
}


extern "C" int fsdf_accum_len(const fsdf_ctx* c, int32_t* len) {
  if (!c || !len) return FSDF_ERR_ARG;
  *len = accum_len(c);
  return FSDF_OK;
}

extern "C" int fsdf_num_points(const fsdf_ctx* c, int64_t* n) {
  if (!c || !n) return FSDF_ERR_ARG;
  *n = c->n;
  return FSDF_OK;
}

static decltype(fsdf_ctx::mech) fresh_mechanism() { return {}; }

// a host array of the model into its (emptied) device buffer of at least min_n
// elements: kernels receive some of these pointers even when the array is
// empty; an empty array without a minimum keeps a null pointer
template <typename T>
static hipError_t upload(fsdf::DevBuf<T>& b, const std::vector<T>& v, size_t min_n = 0) {
  const size_t n = std::max(v.size(), min_n);
  if (n == 0) return hipSuccess;
  const hipError_t e = b.reserve(n);
  if (e != hipSuccess || v.empty()) return e;
  return hipMemcpy(b.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

extern "C" int fsdf_set_surfaces(fsdf_ctx* c, const fsdf_surface* surfs, int32_t S) {
  if (!c) return FSDF_ERR_ARG;
  if (!surfs || S < 1) return fail(c, FSDF_ERR_ARG, "set_surfaces: need at least one surface");
  if (S > fsdf::kMaxHulls) return fail(c, FSDF_ERR_ARG, "set_surfaces: %d surfaces exceeds the limit %d", S, fsdf::kMaxHulls);
  std::vector<fsdf_hull> hulls;
  std::vector<int32_t> hull_surface, surface_kind, rbf_surface, rbf_row_off{0}, rbf_acc_off{0};
  for (int k = 0; k < S; ++k) {
    surface_kind.push_back(surfs[k].kind);
    if (surfs[k].kind == FSDF_SURFACE_HULL) {
      hulls.push_back(surfs[k].hull);
      hull_surface.push_back(k);
    } else if (surfs[k].kind == FSDF_SURFACE_RBF) {
      if (surfs[k].n_centers < 1) return fail(c, FSDF_ERR_ARG, "set_surfaces: RBF surface %d has no centres", k);
      rbf_surface.push_back(k);
      rbf_row_off.push_back(rbf_row_off.back() + surfs[k].n_centers + 1);
      rbf_acc_off.push_back(rbf_acc_off.back() + 4 * surfs[k].n_centers + 4);
    } else {
      return fail(c, FSDF_ERR_ARG, "set_surfaces: surface %d has unknown kind %d", k, surfs[k].kind);
    }
  }
  if (rbf_acc_off.back() > fsdf::kMaxRbfAccum)
    return fail(c, FSDF_ERR_ARG, "set_surfaces: RBF skins need %d accumulators, limit %d", rbf_acc_off.back(),
                fsdf::kMaxRbfAccum);
  const int K = (int)hulls.size();
  std::vector<double> verts, planes, sph, box;
  std::vector<int32_t> faces, face_hull, face_off, vert_hull, vert_off, face_rows;
  int stage_bytes = 0, stage_p64 = 0;
  const int tsz_ = c->precision == 64 ? (int)sizeof(double) : (int)sizeof(float);
  face_off.push_back(0);
  vert_off.push_back(0);
  for (int k = 0; k < K; ++k) {
    const fsdf_hull& h = hulls[(size_t)k];
    if (h.n_vertices < 4 || h.n_faces < 4 || !h.vertices || !h.faces)
      return fail(c, FSDF_ERR_ARG, "set_model: hull %d has %d vertices / %d faces", k, h.n_vertices, h.n_faces);
    const int vbase = (int)(verts.size() / 3);
    double cen[3] = {0, 0, 0};
    for (int i = 0; i < h.n_vertices; ++i)
      for (int j = 0; j < 3; ++j) {
        const double v = h.vertices[3 * i + j];
        if (!std::isfinite(v)) return fail(c, FSDF_ERR_ARG, "set_model: hull %d vertex %d not finite", k, i);
        verts.push_back(v);
        cen[j] += v;
      }
    for (int j = 0; j < 3; ++j) cen[j] /= h.n_vertices;
    for (int i = 0; i < h.n_vertices; ++i) vert_hull.push_back(k);
    vert_off.push_back((int32_t)vert_hull.size());
    double r2 = 0;
    for (int i = 0; i < h.n_vertices; ++i) {
      double s = 0;
      for (int j = 0; j < 3; ++j) {
        const double e = h.vertices[3 * i + j] - cen[j];
        s += e * e;
      }
      r2 = std::max(r2, s);
    }
    // radius padded and rounded up to float: the culling bound stays exact-safe
    float rf = (float)(sqrt(r2) * (1.0 + 1e-9) + 1e-12);
    rf = nextafterf(rf, INFINITY);
    sph.push_back(cen[0]);
    sph.push_back(cen[1]);
    sph.push_back(cen[2]);
    sph.push_back((double)rf);
    // body-frame bounding box, half extents padded and rounded up to float
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < h.n_vertices; ++i)
      for (int j = 0; j < 3; ++j) {
        lo[j] = std::min(lo[j], h.vertices[3 * i + j]);
        hi[j] = std::max(hi[j], h.vertices[3 * i + j]);
      }
    for (int j = 0; j < 3; ++j) box.push_back(0.5 * (lo[j] + hi[j]));
    box.push_back(0.0);
    for (int j = 0; j < 3; ++j) {
      const double c = 0.5 * (lo[j] + hi[j]);
      const double e = std::max(hi[j] - c, c - lo[j]);
      box.push_back((double)nextafterf((float)(e * (1.0 + 1e-9) + 1e-12), INFINITY));
    }
    box.push_back(0.0);
    for (int f = 0; f < h.n_faces; ++f) {
      for (int j = 0; j < 3; ++j) {
        const int vi = h.faces[3 * f + j];
        if (vi < 0 || vi >= h.n_vertices)
          return fail(c, FSDF_ERR_ARG, "set_model: hull %d face %d vertex index %d out of range", k, f, vi);
        faces.push_back(vbase + vi);
      }
      double pl[4];
      if (h.planes) {
        for (int j = 0; j < 4; ++j) pl[j] = h.planes[4 * f + j];
      } else {
        const double* a = h.vertices + 3 * h.faces[3 * f];
        const double* b = h.vertices + 3 * h.faces[3 * f + 1];
        const double* cc = h.vertices + 3 * h.faces[3 * f + 2];
        const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        const double ac[3] = {cc[0] - a[0], cc[1] - a[1], cc[2] - a[2]};
        double nn[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
        const double l = sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
        if (!(l > 0)) return fail(c, FSDF_ERR_DEGENERATE, "set_model: hull %d face %d degenerate", k, f);
        for (int j = 0; j < 3; ++j) pl[j] = nn[j] / l;
        pl[3] = pl[0] * a[0] + pl[1] * a[1] + pl[2] * a[2];
      }
      for (int j = 0; j < 4; ++j) planes.push_back(pl[j]);
      face_hull.push_back(k);
    }
    // face adjacency across each edge v_i -> v_{i+1} (the twin edge's face);
    // an open mesh edge points back at its own face (the certificate then
    // simply fails over to the exhaustive scan). Packed with the face's
    // hull-local vertex indices into one 16-byte row (fsdf_internal.h).
    {
      if (h.n_vertices > 0xffff || h.n_faces > 0xffff)
        return fail(c, FSDF_ERR_ARG, "set_model: hull %d has %d vertices / %d faces (limit 65535)", k,
                    h.n_vertices, h.n_faces);
      std::map<std::pair<int, int>, int> owner;
      for (int f = 0; f < h.n_faces; ++f)
        for (int e = 0; e < 3; ++e) owner[{h.faces[3 * f + e], h.faces[3 * f + (e + 1) % 3]}] = f;
      // exact duplicate planes (coplanar triangles of one facet): a later face
      // with the bitwise plane of an earlier one can never be the first-index
      // maximum, so the fp32 screen leaves it out (no near-tie fallbacks)
      std::map<std::array<uint64_t, 4>, int> seen_plane;
      for (int f = 0; f < h.n_faces; ++f) {
        std::array<uint64_t, 4> key;
        memcpy(key.data(), planes.data() + planes.size() - 4 * (size_t)(h.n_faces - f), sizeof(key));
        const bool dup = !seen_plane.emplace(key, f).second;
        int nb[3];
        for (int e = 0; e < 3; ++e) {
          auto it = owner.find({h.faces[3 * f + (e + 1) % 3], h.faces[3 * f + e]});
          nb[e] = it == owner.end() ? f : it->second;
        }
        const int* fv = h.faces + 3 * f;
        face_rows.push_back((int32_t)((uint32_t)fv[0] | ((uint32_t)fv[1] << 16)));
        face_rows.push_back((int32_t)((uint32_t)fv[2] | ((uint32_t)nb[0] << 16)));
        face_rows.push_back((int32_t)((uint32_t)nb[1] | ((uint32_t)nb[2] << 16)));
        face_rows.push_back(dup ? 1 : 0);
      }
      // per-wave LDS stage: plane rows (f64 contexts: the fp32 screening
      // pairs, 32 B per two faces) and vertex rows of 4 T, one 16-byte face row
      // per face (M64 f64: 4864 B; 4 waves + the wrench rows + the hull table
      // stay under 40 KiB, i.e. 4 workgroups per CU)
      const int plane_bytes = tsz_ == 8 ? 32 * ((h.n_faces + 1) / 2) : h.n_faces * 4 * tsz_;
      stage_bytes = std::max(stage_bytes, plane_bytes + h.n_vertices * 4 * tsz_ + 16 * h.n_faces);
      // (+ the fp64 planes, 32 B per face, when they are staged too; the
      // stage is then a copy of the hull's stage image, whose pair region is
      // nf + 1 chunks as in screen_w)
      stage_p64 = std::max(stage_p64, 16 * (h.n_faces + 1) + h.n_faces * 32 + h.n_vertices * 4 * tsz_ +
                                          16 * h.n_faces);
    }
    face_off.push_back((int32_t)(face_hull.size()));
  }
  // the RBF centre rows are staged through the same buffer, 64 rows at a time
  // at least; the resident-order gradient store transposes 64 x 3 doubles in it
  auto finish_stage = [&](int b) {
    b = (std::max(b, 64 * 4 * std::max(tsz_, 8)) + 15) & ~15;
    if (S <= 64 && rbf_surface.empty())
      b = std::max(b, fsdf::kRedInStageMinBytes);  // wrench rows + transpose after the evaluation
    return b;
  };
  stage_bytes = finish_stage(stage_bytes);
  stage_p64 = finish_stage(stage_p64);
  // f64 hull-only scenes of <= 64 surfaces also stage the fp64 planes when the
  // one-chunk-per-wave pass (wrench rows in the stage) then still runs 4
  // workgroups per CU
  int planes64 = 0;
  if (tsz_ == 8 && S <= 64 && rbf_surface.empty()) {
    fsdf::LocalModel probe;
    probe.K = K;
    probe.S = S;
    probe.stage_bytes = stage_p64;
    // (4 waves per SIMD: 16 waves per CU = 16·64/kPassBlock workgroups)
    if (fsdf::pass_lds_bytes(probe, false, true) <= (size_t)fsdf::kLdsPerCu * fsdf::kPassBlock / 1024 &&
        fsdf::pass_lds_bytes(probe, false) <= (size_t)fsdf::kMaxLds) {
      planes64 = 1;
      stage_bytes = stage_p64;
    }
  }
  {
    fsdf::LocalModel probe;
    probe.K = K;
    probe.S = S;
    probe.R = (int)rbf_surface.size();
    probe.stage_bytes = stage_bytes;
    const size_t lds = fsdf::pass_lds_bytes(probe, false);
    if (lds > (size_t)fsdf::kMaxLds)
      return fail(c, FSDF_ERR_ARG,
                  "set_model: the largest hull needs %d bytes of LDS stage per wave (%zu per workgroup, limit %d); "
                  "decimate it",
                  stage_bytes, lds, fsdf::kMaxLds);
  }
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  free_model(c);
  const int F = (int)face_hull.size(), V = (int)(verts.size() / 3), R = (int)rbf_surface.size();
  const int nrows = rbf_row_off.back();
  const size_t tsz = point_bytes(c);
  std::vector<int32_t> item_meta;  // (LocalModel::item_meta)
  item_meta.reserve((size_t)(F + V) * 4);
  auto meta = [&](int h) {
    const int nf = face_off[h + 1] - face_off[h];
    item_meta.insert(item_meta.end(), {hull_surface[h] | (nf << 16), h, face_off[h], vert_off[h]});
  };
  for (int f = 0; f < F; ++f) meta(face_hull[f]);
  for (int v = 0; v < V; ++v) meta(vert_hull[v]);
  ModelBuffers& mb = c->model;
  HIPCHECK(c, upload(mb.verts_l, verts));
  HIPCHECK(c, upload(mb.faces, faces));
  HIPCHECK(c, upload(mb.planes_l, planes));
  HIPCHECK(c, upload(mb.face_hull, face_hull));
  HIPCHECK(c, upload(mb.sphere_l, sph));
  HIPCHECK(c, upload(mb.box_l, box));
  HIPCHECK(c, upload(mb.face_off, face_off));
  HIPCHECK(c, upload(mb.vert_hull, vert_hull));
  HIPCHECK(c, upload(mb.vert_off, vert_off));
  HIPCHECK(c, upload(mb.face_rows, face_rows, 4));
  HIPCHECK(c, upload(mb.item_meta, item_meta, 4));
  HIPCHECK(c, upload(mb.hull_surface, hull_surface, 1));
  HIPCHECK(c, upload(mb.surface_kind, surface_kind));
  HIPCHECK(c, upload(mb.rbf_surface, rbf_surface, 1));
  HIPCHECK(c, upload(mb.rbf_row_off, rbf_row_off));
  HIPCHECK(c, upload(mb.rbf_acc_off, rbf_acc_off));
  HIPCHECK(c, mb.poses.reserve((size_t)S * 12));
  HIPCHECK(c, mb.accum.reserve((size_t)(1 + 6 * S + rbf_acc_off.back())));
  // per-hull stage images (fsdf_internal.h PosedModel::image_w): the pose
  // kernel rewrites the pairs, planes and vertex rows every pass; the face
  // rows are static and written here
  const size_t chunks = (size_t)4 * F + K + 2 * (size_t)V;
  std::vector<int32_t> img(planes64 ? chunks * 4 : 0, 0);
  for (int h = 0; planes64 && h < K; ++h) {
    const int nf = face_off[h + 1] - face_off[h], nv = vert_off[h + 1] - vert_off[h];
    const size_t base = (size_t)4 * face_off[h] + h + 2 * (size_t)vert_off[h] + 3 * (size_t)nf + 1 + 2 * (size_t)nv;
    memcpy(img.data() + 4 * base, face_rows.data() + 4 * (size_t)face_off[h], (size_t)nf * 4 * sizeof(int32_t));
  }
  auto room = [](auto& buf, size_t n) { return n ? buf.reserve(n) : hipSuccess; };  // (an empty array: no buffer)
  PosedBuffers& pb = c->posed;
  HIPCHECK(c, room(pb.verts_w, (size_t)V * 4 * tsz));
  HIPCHECK(c, pb.planes_w.reserve((size_t)std::max(F, 1) * 4 * tsz));
  // (row K is the sentinel; zeroed here for scenes without hulls, which no pose launch writes)
  HIPCHECK(c, pb.hull_rows.reserve((size_t)(K + 1) * fsdf::kHullRowBytes));
  if (K == 0) HIPCHECK(c, hipMemset(pb.hull_rows.get(), 0, fsdf::kHullRowBytes));
  HIPCHECK(c, pb.screen_w.reserve((size_t)std::max(F + K, 1) * 4));
  if (planes64) {
    HIPCHECK(c, pb.image_w.reserve(chunks * 16));
    HIPCHECK(c, hipMemcpy(pb.image_w.get(), img.data(), chunks * 16, hipMemcpyHostToDevice));
  }
  if (R > 0) {
    HIPCHECK(c, mb.rbf64.reserve((size_t)nrows * 4));
    if (c->precision != 64) HIPCHECK(c, c->rbf32.reserve((size_t)nrows * 4));
    for (int i = 0; i < kPoseRing; ++i) {
      HIPCHECK(c, c->h_rbf[i].reserve((size_t)nrows * 4));
      if (!c->rbf_ev[i]) HIPCHECK(c, c->rbf_ev[i].create(hipEventDisableTiming | hipEventDisableSystemFence));
    }
  }
  for (int i = 0; i < kPoseRing; ++i) {
    c->h_poses[i].reset();  // (the surface count changed: sized anew)
    HIPCHECK(c, c->h_poses[i].reserve((size_t)S * 12));
    if (!c->pose_ev[i]) HIPCHECK(c, c->pose_ev[i].create(hipEventDisableTiming | hipEventDisableSystemFence));
  }
  // every buffer is reserved: the views the kernels take
  fsdf::LocalModel& lm = c->lm;
  lm.K = K;
  lm.F = F;
  lm.V = V;
  lm.S = S;
  lm.R = R;
  lm.rbf_rows = nrows;
  lm.rbf_acc = rbf_acc_off.back();
  lm.stage_bytes = stage_bytes;
  lm.planes64 = planes64;
  lm.verts_l = mb.verts_l.get();
  lm.faces = mb.faces.get();
  lm.planes_l = mb.planes_l.get();
  lm.face_hull = mb.face_hull.get();
  lm.sphere_l = mb.sphere_l.get();
  lm.box_l = mb.box_l.get();
  lm.face_off = mb.face_off.get();
  lm.vert_hull = mb.vert_hull.get();
  lm.vert_off = mb.vert_off.get();
  lm.face_rows = mb.face_rows.get();
  lm.item_meta = mb.item_meta.get();
  lm.hull_surface = mb.hull_surface.get();
  lm.surface_kind = mb.surface_kind.get();
  lm.rbf_surface = mb.rbf_surface.get();
  lm.rbf_row_off = mb.rbf_row_off.get();
  lm.rbf_acc_off = mb.rbf_acc_off.get();
  c->pm.planes_w = pb.planes_w.get();
  c->pm.hull_rows = pb.hull_rows.get();
  c->pm.verts_w = pb.verts_w.get();
  c->pm.screen_w = pb.screen_w.get();
  c->pm.image_w = pb.image_w.get();
  // per-pass RBF rows (f64 contexts read the f64 rows)
  c->pm.rbf_rows = c->precision == 64 ? (void*)mb.rbf64.get() : (void*)c->rbf32.get();
  c->h_surface_kind = surface_kind;
  c->h_n_centers.assign(S, 0);
  for (int k = 0; k < S; ++k) c->h_n_centers[k] = surfs[k].kind == FSDF_SURFACE_RBF ? surfs[k].n_centers : 0;
  // the mechanism's surface bodies / frames / poses and the RBF centre
  // declarations refer to the previous surface list: drop them all (the
  // caller re-registers with fsdf_set_mechanism; iterations fail until then)
  c->mech = fresh_mechanism();
  return FSDF_OK;
}

extern "C" int fsdf_set_model(fsdf_ctx* c, const fsdf_hull* hulls, int32_t K) {
  if (!c) return FSDF_ERR_ARG;
  if (!hulls || K < 1) return fail(c, FSDF_ERR_ARG, "set_model: need at least one hull");
  std::vector<fsdf_surface> s((size_t)K);
  for (int k = 0; k < K; ++k) {
    s[(size_t)k].kind = FSDF_SURFACE_HULL;
    s[(size_t)k].n_centers = 0;
    s[(size_t)k].hull = hulls[k];
  }
  return fsdf_set_surfaces(c, s.data(), K);
}

extern "C" int fsdf_set_rbf_params(fsdf_ctx* c, const double* params, int64_t n) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.R == 0) return fail(c, FSDF_ERR_STATE, "set_rbf_params: the scene has no RBF surface");
  if (!params || n != 4LL * c->lm.rbf_rows)
    return fail(c, FSDF_ERR_ARG, "set_rbf_params: expected %d doubles, got %lld", 4 * c->lm.rbf_rows, (long long)n);
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(params[i])) return fail(c, FSDF_ERR_ARG, "set_rbf_params: entry %lld not finite", (long long)i);
  HIPCHECK(c, hipSetDevice(c->device));
  // own ring: the slot is reused only after the copy that last read it ran
  // (the ring events only mark a copy's completion: no system-scope fence)
  // (an asynchronous caller may queue several passes with different rows)
  const int sl = c->rbf_slot;
  c->rbf_slot = (sl + 1) % kPoseRing;
  HIPCHECK(c, hipEventSynchronize(c->rbf_ev[sl]));
  memcpy(c->h_rbf[sl].get(), params, (size_t)n * sizeof(double));
  HIPCHECK(c, hipMemcpyAsync(c->model.rbf64.get(), c->h_rbf[sl].get(), (size_t)n * sizeof(double),
                             hipMemcpyHostToDevice, c->stream));
  HIPCHECK(c, hipEventRecord(c->rbf_ev[sl], c->stream));
  if (c->precision != 64) HIPCHECK(c, fsdf::launch_to_f32(c->model.rbf64.get(), c->rbf32.get(), n, c->stream));
  c->rbf_ready = true;
  return FSDF_OK;
}

extern "C" int fsdf_set_partition(fsdf_ctx* c, int64_t four_way_max_points, int64_t two_way_max_points) {
  if (!c) return FSDF_ERR_ARG;
  if (four_way_max_points < -1 || two_way_max_points < -1)
    return fail(c, FSDF_ERR_ARG, "set_partition: limits are -1 (model default), 0 (off) or a point count");
  c->lm.hpart4_points = four_way_max_points;
  c->lm.hpart2_points = two_way_max_points;
  return FSDF_OK;
}

extern "C" int fsdf_get_partition(fsdf_ctx* c, int64_t n, int64_t* four_way_max_out, int64_t* two_way_max_out,
                                  int32_t* parts_out) {
  if (!c) return FSDF_ERR_ARG;
  int64_t f4, f2;
  fsdf::hpart_default_limits(c->lm, &f4, &f2);
  if (c->lm.hpart4_points >= 0) f4 = c->lm.hpart4_points;
  if (c->lm.hpart2_points >= 0) f2 = c->lm.hpart2_points;
  if (four_way_max_out) *four_way_max_out = f4;
  if (two_way_max_out) *two_way_max_out = f2;
  if (parts_out) *parts_out = c->lm.K > 0 ? fsdf::hpart_parts(c->lm, n) : 0;
  return FSDF_OK;
}

extern "C" const char* fsdf_pass_kernel_name(const fsdf_ctx* c) { return c ? c->pass_kernel.c_str() : ""; }

extern "C" int fsdf_chunk_costs(fsdf_ctx* c, uint32_t* costs_out, int64_t* count_out) {
  if (!c || !count_out) return FSDF_ERR_ARG;
  // a regrouped range's chunks are no longer the whole cloud's Hilbert chunks:
  // costs balanced as if they were would place the cut by wrong prefix sums
  if (c->ranged && c->regrouped)
    return fail(c, FSDF_ERR_STATE, "chunk_costs: the ranged cloud was regrouped (its chunks are not the whole "
                                   "cloud's order); gather costs before fsdf_regroup_points");
  const int64_t nc = c->plan_nc > 0 ? c->plan_nc : 0;
  *count_out = nc;
  if (!costs_out || nc == 0) return FSDF_OK;
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  HIPCHECK(c, hipMemcpy(costs_out, c->chunk.dur.get(), (size_t)nc * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return FSDF_OK;
}

extern "C" int fsdf_set_plan(fsdf_ctx* c, int32_t enable, double four_way_share, double two_way_share,
                             int64_t max_points) {
  if (!c) return FSDF_ERR_ARG;
  if (!(four_way_share <= 1.0 && two_way_share <= 1.0) || four_way_share != four_way_share || two_way_share != two_way_share)
    return fail(c, FSDF_ERR_ARG, "set_plan: shares must lie in [0, 1] (or < 0: the default counts)");
  if (max_points < -1) return fail(c, FSDF_ERR_ARG, "set_plan: max_points is -1 (default) or a point count");
  c->plan_enable = enable != 0;
  c->plan_f4 = four_way_share;
  c->plan_f2 = two_way_share;
  c->plan_max_points = max_points < 0 ? -1 : max_points;
  c->plan_nc = -1;  // rebuilt on the next pass
  return FSDF_OK;
}

extern "C" int fsdf_set_output_order(fsdf_ctx* c, int32_t order) {
  if (!c) return FSDF_ERR_ARG;
  if (order != FSDF_ORDER_CALLER && order != FSDF_ORDER_RESIDENT)
    return fail(c, FSDF_ERR_ARG, "set_output_order: unknown order %d", order);
  c->out_order = order;
  return FSDF_OK;
}

extern "C" int fsdf_skin(fsdf_ctx* c, const double* poses, const double* xyz, int64_t n, double* d_out,
                         int32_t* kstar_out, double* grad_out) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "skin: no model (call fsdf_set_model first)");
  if (!poses || n < 0 || (n > 0 && !xyz)) return fail(c, FSDF_ERR_ARG, "skin: bad arguments");
  HIPCHECK(c, hipSetDevice(c->device));
  if (n == 0) return FSDF_OK;
  int rc = ensure_outputs(c, n);
  if (rc) return rc;
  // stage the query points (f64 on the device, then the context precision)
  if (c->q64.capacity() < (size_t)n * 3) HIPCHECK(c, hipStreamSynchronize(c->stream));
  HIPCHECK(c, c->q64.reserve((size_t)n * 3));
  HIPCHECK(c, hipMemcpyAsync(c->q64.get(), xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const void* d_query = c->q64.get();
  if (c->precision != 64) {
    rc = adopt_points_device(c, c->q64.get(), n, c->q);
    if (rc) return rc;
    d_query = c->q.get();
  }
  rc = run_pass(c, poses, d_query, n, c->model.accum.get(), c->kstar.get(), c->d.get(), c->grad.get(), nullptr,
                false);
  if (rc) return rc;
  return fetch(c, n, nullptr, nullptr, kstar_out, d_out, grad_out, true);
}

extern "C" int fsdf_synchronize(fsdf_ctx* c) {
  if (!c) return FSDF_ERR_ARG;
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}

extern "C" int fsdf_profile_pass(fsdf_ctx* c, int32_t enable) {
  if (!c) return FSDF_ERR_ARG;
  HIPCHECK(c, hipSetDevice(c->device));
  if (enable && c->prof_ev.empty()) {
    c->prof_ev.resize(3 * 4096);
    // timing-only events: a default event record is a system-scope release
    // (the whole L2 written back), which put ~10 us between the pass and the
    // reduce of every profiled pass; fsdf_pass_times synchronizes the stream
    // before reading them
    for (auto& e : c->prof_ev) HIPCHECK(c, e.create(hipEventDisableSystemFence));
  }
  if (enable && c->skin_ev.empty() && c->lm.R > 0) {
    c->skin_ev.resize(2 * 256);
    for (auto& e : c->skin_ev) HIPCHECK(c, e.create(hipEventDisableSystemFence));
  }
  c->profiling = enable != 0;
  c->prof_used = 0;
  c->skin_ev_used = 0;
  c->score_ev_used = 0;  // (fsdf_score_time's pairs: created by the first profiled scoring call)
  return FSDF_OK;
}

extern "C" int fsdf_pass_times(fsdf_ctx* c, double* kernel_ms, double* pass_ms, int64_t* launches) {
  if (!c || !kernel_ms || !pass_ms || !launches) return FSDF_ERR_ARG;
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  double tk = 0.0, tp = 0.0;
  for (size_t i = 0; i + 2 < c->prof_used; i += 3) {
    float k = 0.f, p = 0.f;
    HIPCHECK(c, hipEventElapsedTime(&k, c->prof_ev[i], c->prof_ev[i + 1]));
    HIPCHECK(c, hipEventElapsedTime(&p, c->prof_ev[i], c->prof_ev[i + 2]));
    tk += k;
    tp += p;
  }
  *kernel_ms = tk;
  *pass_ms = tp;
  *launches = (int64_t)(c->prof_used / 3);
  c->prof_used = 0;
  return FSDF_OK;
}

extern "C" int fsdf_pass_time(fsdf_ctx* c, double* total_ms, int64_t* launches) {
  double k = 0.0;
  return fsdf_pass_times(c, &k, total_ms, launches);
}

// 24 counters; diagnostic builds with -DFSDF_WAVE_TIMES=1 append per-wave clocks
static constexpr int kStatCount = FSDF_WAVE_TIMES ? 32 + 32 * fsdf::kMaxBlocks : 24;

extern "C" int fsdf_kernel_stats(fsdf_ctx* c, int32_t enable, uint64_t* counters) {
  if (!c) return FSDF_ERR_ARG;
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, c->stats.reserve(kStatCount));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  if (enable) {
    HIPCHECK(c, hipMemset(c->stats.get(), 0, kStatCount * sizeof(unsigned long long)));
    c->stats_on = true;
    return FSDF_OK;
  }
  c->stats_on = false;
  if (counters) HIPCHECK(c, hipMemcpy(counters, c->stats.get(), kStatCount * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return FSDF_OK;
}

extern "C" int fsdf_raycast(fsdf_ctx* c, const double* poses, const double* origin, const double* rays, int64_t n,
                            double* depth_out) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "raycast: no model (call fsdf_set_surfaces first)");
  if (!poses || !origin || n < 0 || (n > 0 && (!rays || !depth_out))) return fail(c, FSDF_ERR_ARG, "raycast: bad arguments");
  if (c->lm.R > 0 && !c->rbf_ready)
    return fail(c, FSDF_ERR_STATE, "raycast: the scene has RBF surfaces: call fsdf_set_rbf_params first");
  for (int j = 0; j < 3; ++j)
    if (!std::isfinite(origin[j])) return fail(c, FSDF_ERR_ARG, "raycast: origin not finite");
  HIPCHECK(c, hipSetDevice(c->device));
  if (n == 0) return FSDF_OK;
  int rc = ensure_outputs(c, n);
  if (rc) return rc;
  if (c->q64.capacity() < (size_t)n * 3) HIPCHECK(c, hipStreamSynchronize(c->stream));
  HIPCHECK(c, c->q64.reserve((size_t)n * 3));
  HIPCHECK(c, hipMemcpyAsync(c->q64.get(), rays, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  rc = pose_model(c, poses);
  if (rc) return rc;
  HIPCHECK(c, fsdf::launch_raycast(c->precision, c->cull != 0, c->lm, c->pm, origin, c->q64.get(), n, c->d.get(),
                                   c->stream));
  HIPCHECK(c, hipMemcpyAsync(depth_out, c->d.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}
