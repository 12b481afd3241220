// Rollout frames rasterised on the GPU (dgppo_render_frames): the drawing half of the reference's render_video
// (dgppo/env/plot.py render_lidar / render_mpe) as ONE launch over (frame, pixel tile).
//
// Pixel rule (DESIGN.md "Rendering"): the world square [0, L]^2 maps onto S x S pixels of pitch h = L / S, pixel
// (row, col) samples p = ((col + 0.5) h, (S - row - 0.5) h); every shape has a signed distance d(p), its coverage is
// clamp(0.5 - d / h, 0, 1), and the shapes are composited in painter's order in fp32 on straight sRGB values,
// c += alpha * cov * (col - c) from white; the stored byte is floor(255 c + 0.5), A = 255.
//
// A 256-thread workgroup owns one 32 x 32 pixel tile of one frame (4 pixels per thread; a wave stores two rows of 32
// adjacent pixels, 128 contiguous bytes each).  The frame's primitives -- MPE obstacle circles, FoV wedges, edges, goal
// and agent circles, Lidar rectangles, in that order -- are numbered 0 .. P-1 and processed in chunks of 256: thread i
// builds primitive chunk * 256 + i from the state rows, drops it when it is invalid (pad / out-of-range edge index,
// non-finite coordinate), when its bounding box, grown by one pixel pitch, misses the tile's pixel centres, or when its
// signed distance at the tile's centre exceeds the tile's half-diagonal by more than one pixel pitch, and a ballot /
// prefix rank compacts the survivors IN ORDER into an LDS list; after a barrier every pixel walks the list (all lanes
// read the same entry: LDS broadcasts).  A dropped primitive has d >= h on every pixel centre of the tile (d is bounded
// below by the distance to its bounding circle / box, and the four signed distances are exact, hence 1-Lipschitz),
// i.e. coverage exactly 0, so culling never changes a byte.  No atomics, no data-dependent ordering: two launches give
// identical bytes.
//
// Layer 0, optional (dgppo_render_frames_field): a scalar field on a uniform Gx x Gy grid, drawn UNDER every other
// layer -- the reference's contourf + zero-level contour (plot.py viz_opts["cbf"]) by this project's own rule.  A
// pixel centre inside the grid's extent interpolates its cell's four nodes bilinearly, takes one of K hard-edged
// bands of a red-to-blue palette (staged in LDS) at alpha 0.9 on white, and is then covered by the black zero line
// where |val| / |grad val|, the first-order distance to the zero level, is within the line's half-width.  A pixel
// outside the extent, or in a cell with a non-finite node, stays white.  The pixel loop then starts from that colour.
//
// The VMAS envs (dgppo_render_frames_vmas; the reference's vmas_wheel.py / vmas_reverse_transport.py render_video) are
// a third compile-time form of the same tile code, render_kernel<false, true>: the view is the square of side
// V = 2 m hw about the ORIGIN (hw = area_size / 2, m = 1.02 Wheel / 1.01 Transport, h = V / S,
// p = (-V/2 + (col + 0.5) h, V/2 - (row + 0.5) h)), build_vmas() makes the frame's 7 (Wheel) or 10 (Transport)
// primitives from the four state rows and the env record, and a primitive carries its own 24-bit colour (matplotlib's
// C0 .. C5) in `kind`, so Prim stays 32 B.
// One new shape, the rectangle OUTLINE: d = |d_rect| - half_width.  |.| of a 1-Lipschitz function is 1-Lipschitz, so
// d is, and d >= (distance to the rectangle grown by half_width) >= (distance to the circle of radius
// sqrt(hw^2 + hh^2) + half_width about its centre); the box cull uses that circle's box grown by one pitch and the
// centre cull the exact d, so the argument above holds unchanged: a dropped outline has d >= h on every pixel centre of
// the tile, coverage exactly 0.  The avoid sector is the wedge distance with the launch's radius and half-angle; cos /
// sin of the three angles are taken once per primitive in build_vmas(), never per pixel.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/dgppo_hip.h"
#include "vmas.h"

namespace dgppo {
namespace {

constexpr int kThreads = 256, kTileW = 32, kTileH = 32, kPix = kTileW * kTileH / kThreads;  // 4 rows per thread
constexpr int kRowStep = kThreads / kTileW;  // rows between a thread's pixels
constexpr int kCircle = 0, kRect = 1, kEdge = 2, kWedge = 3, kOutline = 4;  // kOutline: VMAS form only
// colours: 0 obstacle #8a0000, 1 agent / wedge #0068ff, 2 goal / goal edge #2fdd00, 3 edge #333333
constexpr int kRed = 0, kBlue = 1, kGreen = 2, kGrey = 3;

struct Prim {        // 32 B
  float a[6];        // circle: cx cy r | rect: cx cy w/2 h/2 cos sin | edge: ax ay bx by | wedge: cx cy hx hy (unit)
  int32_t kind;      // shape | colour << 8; VMAS form: shape | 0xRRGGBB << 4 (the colour itself; < 2^28, so >= 0)
  float alpha;
};

struct Params {
  const float* states;
  const int32_t* receivers;
  const int32_t* senders;
  const float* obstacles;
  uint32_t* out;
  int64_t s_es, s_ts, i_es, i_ts, o_es;
  int32_t fpe, S, tiles_x, tiles_per_frame;
  int32_t n, ng, O, N, E, sd;
  int32_t nA, nB, nC, nD, nE;  // primitives per layer: MPE circles, wedges, edges, goal + agent circles, rectangles
  float L, h, inv_h, car_r, obs_r, fov_r, sin_b, cos_b, edge_hw;
  // layer 0 (render_kernel<true> only): frame f reads the (gy, gx) nodes at field + f * gy * gx
  const float* field;
  const float* palette;  // (bands, 3)
  int32_t gx, gy, bands;
  float fx0, fy0, inv_dx, inv_dy, f_half, inv_band, f_alpha, line_hw, grad_eps;
  // VMAS form only; at the end, so the other two kernels read their arguments where they did
  int32_t wheel, vmas_prims;  // engine is VMASWheel; primitives per frame
  float half_view, outline_hw, goal_r, box_centre_r;  // V / 2; V / 1440; dist2goal; dist2goal / 2
};

__device__ __forceinline__ bool fin(float x) { return fabsf(x) <= 3.4028234664e38f; }  // false for NaN / inf

// Primitive k of the frame, or kind < 0 when it contributes nothing.  bb = its bounding box [x0, x1, y0, y1].
__device__ __forceinline__ Prim build(const Params& P, const float* __restrict__ st, const int32_t* __restrict__ rc,
                                      const int32_t* __restrict__ sn, const float* __restrict__ ob, int k, float bb[4]) {
  Prim q;
  q.kind = -1;
  q.alpha = 1.0f;
  for (int i = 0; i < 6; ++i) q.a[i] = 0.0f;
  float cx = 0.0f, cy = 0.0f, R = 0.0f;  // bounding circle (edges set bb themselves)
  bool have_bb = false;
  if (k < P.nA) {  // MPE obstacle circle, state row n + ng + k
    const float* s = st + (int64_t)(P.n + P.ng + k) * P.sd;
    cx = s[0], cy = s[1], R = P.obs_r;
    if (fin(cx) && fin(cy)) q.kind = kCircle | (kRed << 8);
    q.a[0] = cx, q.a[1] = cy, q.a[2] = R;
  } else if ((k -= P.nA) < P.nB) {  // FoV wedge of agent k
    const float* s = st + (int64_t)k * P.sd;
    cx = s[0], cy = s[1], R = P.fov_r;
    const float hx = s[2], hy = s[3];
    if (fin(cx) && fin(cy) && fin(hx) && fin(hy)) q.kind = kWedge | (kBlue << 8);
    const float inv = 1.0f / fmaxf(sqrtf(hx * hx + hy * hy), 1e-12f);
    q.a[0] = cx, q.a[1] = cy, q.a[2] = hx * inv, q.a[3] = hy * inv;
    q.alpha = 0.15f;
  } else if ((k -= P.nB) < P.nC) {  // edge k: capsule sender -> receiver
    const int r = rc[k], s = sn[k];
    if (r >= 0 && s >= 0 && r < P.N - 1 && s < P.N - 1) {  // N - 1 is the pad node
      const float* a = st + (int64_t)s * P.sd;
      const float* b = st + (int64_t)r * P.sd;
      const float ax = a[0], ay = a[1], bx = b[0], by = b[1];
      if (fin(ax) && fin(ay) && fin(bx) && fin(by))
        q.kind = kEdge | ((s >= P.n && s < P.n + P.ng ? kGreen : kGrey) << 8);
      q.a[0] = ax, q.a[1] = ay, q.a[2] = bx, q.a[3] = by;
      const float m = P.edge_hw + P.h;
      bb[0] = fminf(ax, bx) - m, bb[1] = fmaxf(ax, bx) + m, bb[2] = fminf(ay, by) - m, bb[3] = fmaxf(ay, by) + m;
      have_bb = true;
    }
    q.alpha = 0.5f;
  } else if ((k -= P.nC) < P.nD) {  // goal circles ng-1 .. 0, then agent circles n-1 .. 0
    const bool goal = k < P.ng;
    const int row = goal ? P.n + (P.ng - 1 - k) : P.n - 1 - (k - P.ng);
    const float* s = st + (int64_t)row * P.sd;
    cx = s[0], cy = s[1], R = P.car_r;
    if (fin(cx) && fin(cy)) q.kind = kCircle | ((goal ? kGreen : kBlue) << 8);
    q.a[0] = cx, q.a[1] = cy, q.a[2] = R;
  } else if ((k -= P.nD) < P.nE) {  // Lidar obstacle rectangle k
    const float* o = ob + (int64_t)k * DGPPO_OBST_FIELDS;
    cx = o[0], cy = o[1];
    const float hw = 0.5f * o[2], hh = 0.5f * o[3], c = o[5], s = o[6];
    if (fin(cx) && fin(cy) && fin(hw) && fin(hh) && fin(c) && fin(s)) q.kind = kRect | (kRed << 8);
    q.a[0] = cx, q.a[1] = cy, q.a[2] = hw, q.a[3] = hh, q.a[4] = c, q.a[5] = s;
    R = sqrtf(hw * hw + hh * hh);
    // the bounds on d hold only for a rotation; records with another (cos, sin) are never culled
    if (!(fabsf(c * c + s * s - 1.0f) <= 1e-3f)) R = INFINITY, q.alpha = -1.0f;
  }
  if (!have_bb) {
    const float m = R + P.h;
    bb[0] = cx - m, bb[1] = cx + m, bb[2] = cy - m, bb[3] = cy + m;
  }
  return q;
}

// matplotlib's default colour cycle as the `kind` bits of a VMAS primitive
constexpr int32_t rgb(int32_t hex) { return hex << 4; }
constexpr int32_t kC0 = rgb(0x1f77b4), kC1 = rgb(0xff7f0e), kC2 = rgb(0x2ca02c), kC3 = rgb(0xd62728),
                  kC4 = rgb(0x9467bd), kC5 = rgb(0x8c564b);
// the reference classes' fixed sizes (vmas_wheel.py:57-60, :337; vmas_reverse_transport.py:57-61)
constexpr float kLineLength = 2.0f, kLineHalfWidth = 0.025f, kBoxHalf = 0.3f, kVmasObsR = 0.15f;

// Primitive k of a VMAS frame in layer order (DESIGN.md "Rendering", the two VMAS tables), as build() does it: kind < 0
// when it contributes nothing, bb its bounding box grown by one pitch.  st: the (4, 4) state rows, rec: the env record.
__device__ __forceinline__ Prim build_vmas(const Params& P, const float* __restrict__ st,
                                           const float* __restrict__ rec, int k, float bb[4]) {
  Prim q;
  q.kind = -1;
  q.alpha = 1.0f;
  for (int i = 0; i < 6; ++i) q.a[i] = 0.0f;
  float cx = 0.0f, cy = 0.0f, R = 0.0f;  // bounding circle
  const int first_agent = P.vmas_prims - (P.wheel ? 3 : 4);  // Transport: the box centre comes after the agents
  if (k >= first_agent && k < first_agent + 3) {  // agent discs 0, 1, 2 (agent 2 on top)
    const int i = k - first_agent;
    const float* s = st + i * P.sd;
    cx = s[0], cy = s[1], R = P.car_r;
    if (fin(cx) && fin(cy)) q.kind = kCircle | (i == 0 ? kC2 : i == 1 ? kC1 : kC4);
    q.a[0] = cx, q.a[1] = cy, q.a[2] = R;
  } else if (P.wheel) {
    const float ang = k == 0 ? rec[1] : k == 3 ? rec[0] : st[3 * P.sd];  // avoid, goal, line angle
    const bool ok = fin(ang);
    const float c = ok ? cosf(ang) : 1.0f, s = ok ? sinf(ang) : 0.0f;
    if (k == 0) {  // avoid sector: the wedge about the origin (radius, half-angle: fov_r, sin_b, cos_b)
      R = P.fov_r;
      if (ok) q.kind = kWedge | kC0;
      q.a[2] = c, q.a[3] = s;
      q.alpha = 0.2f;
    } else if (k == 3) {  // goal ray: capsule origin -> line_length (cos, sin), half-width edge_hw
      R = kLineLength + P.edge_hw;
      if (ok) q.kind = kEdge | kC5;
      q.a[2] = kLineLength * c, q.a[3] = kLineLength * s;
      q.alpha = 0.2f;
    } else {  // k = 1, 2: the line's positive (C5) and negative (C3) half
      const float half = 0.25f * kLineLength, sign = k == 1 ? 1.0f : -1.0f;
      cx = sign * half * c, cy = sign * half * s;
      if (ok) q.kind = kRect | (k == 1 ? kC5 : kC3);
      q.a[0] = cx, q.a[1] = cy, q.a[2] = half, q.a[3] = kLineHalfWidth, q.a[4] = c, q.a[5] = s;
      R = sqrtf(half * half + kLineHalfWidth * kLineHalfWidth);
    }
  } else if (k == 0 || k == 5) {  // arena outline [-hw, hw]^2; box outline about states[3, :2]
    const float* s = st + 3 * P.sd;
    const float half = k == 0 ? 0.5f * P.L : kBoxHalf;
    cx = k == 0 ? 0.0f : s[0], cy = k == 0 ? 0.0f : s[1];
    if (fin(cx) && fin(cy)) q.kind = kOutline | kC3;
    q.a[0] = cx, q.a[1] = cy, q.a[2] = half, q.a[3] = half, q.a[4] = 1.0f, q.a[5] = 0.0f;
    R = 1.41421357f * half + P.outline_hw;  // sqrt(2) rounded up
  } else {  // discs: goal (k = 1), obstacles 0 .. 2 (k = 2 .. 4), box centre (k = 9)
    const float* s = k == 9 ? st + 3 * P.sd : rec + 2 * (k - 1);
    cx = s[0], cy = s[1];
    R = k == 1 ? P.goal_r : k == 9 ? P.box_centre_r : kVmasObsR;
    if (fin(cx) && fin(cy)) q.kind = kCircle | (k == 1 ? kC5 : k == 9 ? kC3 : kC0);
    q.a[0] = cx, q.a[1] = cy, q.a[2] = R;
    q.alpha = k == 1 ? 0.5f : k == 9 ? 1.0f : 0.7f;
  }
  const float m = R + P.h;
  bb[0] = cx - m, bb[1] = cx + m, bb[2] = cy - m, bb[3] = cy + m;
  return q;
}

__device__ __forceinline__ float sgn(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

template <bool kVmas>
__device__ __forceinline__ float distance(const Prim& q, int shape, float px, float py, const Params& P) {
  if (shape == kCircle) {
    const float dx = px - q.a[0], dy = py - q.a[1];
    return sqrtf(dx * dx + dy * dy) - q.a[2];
  }
  if (shape == kEdge) {
    const float pax = px - q.a[0], pay = py - q.a[1], bax = q.a[2] - q.a[0], bay = q.a[3] - q.a[1];
    const float t = fminf(fmaxf((pax * bax + pay * bay) / fmaxf(bax * bax + bay * bay, 1e-12f), 0.0f), 1.0f);
    const float ex = pax - t * bax, ey = pay - t * bay;
    return sqrtf(ex * ex + ey * ey) - P.edge_hw;
  }
  if (shape == kRect || (kVmas && shape == kOutline)) {
    const float dx = px - q.a[0], dy = py - q.a[1], c = q.a[4], s = q.a[5];
    const float qx = fabsf(c * dx + s * dy) - q.a[2], qy = fabsf(c * dy - s * dx) - q.a[3];
    const float ox = fmaxf(qx, 0.0f), oy = fmaxf(qy, 0.0f);
    const float d = sqrtf(ox * ox + oy * oy) + fminf(fmaxf(qx, qy), 0.0f);
    if constexpr (kVmas) {
      if (shape == kOutline) return fabsf(d) - P.outline_hw;
    }
    return d;
  }
  // wedge: exact circular-sector distance in the heading frame, (v, u) = (across, along)
  const float dx = px - q.a[0], dy = py - q.a[1], hx = q.a[2], hy = q.a[3];
  const float u = dx * hx + dy * hy, v = fabsf(dx * hy - dy * hx);
  const float l = sqrtf(u * u + v * v) - P.fov_r;
  const float kk = fminf(fmaxf(v * P.sin_b + u * P.cos_b, 0.0f), P.fov_r);
  const float mv = v - kk * P.sin_b, mu = u - kk * P.cos_b;
  const float m = sqrtf(mv * mv + mu * mu);
  return fmaxf(l, m * sgn(P.cos_b * v - P.sin_b * u));
}

// Layer 0 at pixel centre (px, py): the colour the pixel starts from.  `pal` is the palette in LDS.
__device__ __forceinline__ void field_colour(const Params& P, const float* __restrict__ fv, const float* pal, float px,
                                             float py, float& r, float& g, float& b) {
  const float u = (px - P.fx0) * P.inv_dx, v = (py - P.fy0) * P.inv_dy;
  const float umax = (float)(P.gx - 1), vmax = (float)(P.gy - 1);
  if (!(u >= 0.0f && u <= umax && v >= 0.0f && v <= vmax)) return;  // outside (u, v are finite: the extent is)
  const float fi = fminf(floorf(u), umax - 1.0f), fj = fminf(floorf(v), vmax - 1.0f);  // in [0, g - 2]
  const int i = (int)fi, j = (int)fj;
  const float* c = fv + (int64_t)j * P.gx + i;
  const float v00 = c[0], v10 = c[1], v01 = c[P.gx], v11 = c[P.gx + 1];
  if (!(fin(v00) && fin(v10) && fin(v01) && fin(v11))) return;
  const float tx = u - fi, ty = v - fj;
  const float lo = v00 + tx * (v10 - v00), hi = v01 + tx * (v11 - v01);
  const float val = lo + ty * (hi - lo);
  const float gx = ((v10 - v00) + ty * ((v11 - v01) - (v10 - v00))) * P.inv_dx, gy = (hi - lo) * P.inv_dy;
  const float s = (val + P.f_half) * P.inv_band;
  const int band = (int)fminf(fmaxf(floorf(s), 0.0f), (float)(P.bands - 1));  // NaN -> 0: never out of the palette
  r += P.f_alpha * (pal[3 * band] - r);
  g += P.f_alpha * (pal[3 * band + 1] - g);
  b += P.f_alpha * (pal[3 * band + 2] - b);
  const float gn = sqrtf(gx * gx + gy * gy);
  if (gn * P.L > P.grad_eps) {  // the zero line, black, alpha 1
    const float w = fminf(fmaxf(0.5f - (fabsf(val) / gn - P.line_hw) * P.inv_h, 0.0f), 1.0f);
    r -= w * r;
    g -= w * g;
    b -= w * b;
  }
}

// kVmas: the origin-centred view, build_vmas() and the colour carried in the primitive; receivers / senders are not
// touched.  render_kernel<false> and <true> are the instructions they were before the VMAS form existed.
template <bool kField, bool kVmas = false>
__global__ __launch_bounds__(kThreads) void render_kernel(const Params P) {
  static_assert(!(kField && kVmas), "the VMAS form has no field layer");
  __shared__ Prim list[kThreads];
  __shared__ int wave_count[kThreads / 64];
  __shared__ float pal[3 * DGPPO_RENDER_MAX_BANDS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frame = blockIdx.x / P.tiles_per_frame, tile = blockIdx.x % P.tiles_per_frame;
  const int ty = tile / P.tiles_x, tx = tile % P.tiles_x;
  const int e = frame / P.fpe, t = frame % P.fpe;
  const float* st = P.states + e * P.s_es + t * P.s_ts;
  const int32_t* rc = kVmas ? nullptr : P.receivers + e * P.i_es + t * P.i_ts;
  const int32_t* sn = kVmas ? nullptr : P.senders + e * P.i_es + t * P.i_ts;
  const float* ob = P.obstacles + e * P.o_es;

  // this thread's pixels: column col, rows row0 + kRowStep j
  const int col = tx * kTileW + (tid & (kTileW - 1)), row0 = ty * kTileH + tid / kTileW;
  const float org = kVmas ? P.half_view : 0.0f;  // the world coordinate of the view's left / bottom edge is -org
  float px = ((float)col + 0.5f) * P.h;
  if constexpr (kVmas) px -= org;
  float py[kPix], cr[kPix], cg[kPix], cb[kPix];
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    py[j] = ((float)(P.S - (row0 + kRowStep * j)) - 0.5f) * P.h;
    if constexpr (kVmas) py[j] -= org;
    cr[j] = cg[j] = cb[j] = 1.0f;
  }
  if constexpr (kField) {
    if (tid < 3 * P.bands) pal[tid] = P.palette[tid];
    __syncthreads();
    const float* fv = P.field + (int64_t)frame * P.gy * P.gx;
#pragma unroll
    for (int j = 0; j < kPix; ++j) field_colour(P, fv, pal, px, py[j], cr[j], cg[j], cb[j]);
  }
  // the tile's pixel centres span [x0, x1] x [y0, y1]
  const int c1 = min(tx * kTileW + kTileW, P.S), r1 = min(ty * kTileH + kTileH, P.S);
  float x0 = ((float)(tx * kTileW) + 0.5f) * P.h, x1 = ((float)c1 - 0.5f) * P.h;
  float y1 = ((float)(P.S - ty * kTileH) - 0.5f) * P.h, y0 = ((float)(P.S - r1) + 0.5f) * P.h;
  if constexpr (kVmas) x0 -= org, x1 -= org, y0 -= org, y1 -= org;
  const float mx = 0.5f * (x0 + x1), my = 0.5f * (y0 + y1);
  const float reach = 0.5f * sqrtf((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0)) + P.h;  // half-diagonal + one pitch

  const int total = kVmas ? P.vmas_prims : P.nA + P.nB + P.nC + P.nD + P.nE;
  for (int base = 0; base < total; base += kThreads) {
    const int k = base + tid;
    float bb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    Prim q;
    q.kind = -1;
    if (k < total) {
      if constexpr (kVmas) q = build_vmas(P, st, ob, k, bb);
      else q = build(P, st, rc, sn, ob, k, bb);
    }
    // finiteness was tested in build(); the box test is on floats, nothing is converted to an integer
    bool keep = q.kind >= 0 && !(bb[1] < x0 || bb[0] > x1 || bb[3] < y0 || bb[2] > y1);
    if (keep && q.alpha >= 0.0f)  // NaN keeps
      keep = !(distance<kVmas>(q, q.kind & (kVmas ? 0xf : 0xff), mx, my, P) > reach);
    q.alpha = fabsf(q.alpha);
    const unsigned long long mask = __ballot(keep);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int offset = 0, count = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      const int c = wave_count[w];
      offset += w < wave ? c : 0;
      count += c;
    }
    if (keep) list[offset + rank] = q;
    __syncthreads();
    for (int i = 0; i < count; ++i) {
      const Prim s = list[i];
      const int shape = s.kind & (kVmas ? 0xf : 0xff), colour = s.kind >> (kVmas ? 4 : 8);
      float r, g, b;
      if constexpr (kVmas) {  // 0xRRGGBB
        r = (float)(colour >> 16) / 255.0f, g = (float)((colour >> 8) & 0xff) / 255.0f;
        b = (float)(colour & 0xff) / 255.0f;
      } else {  // #8a0000, #0068ff, #2fdd00, #333333
        r = colour == kRed ? 138 / 255.0f : colour == kBlue ? 0.0f : colour == kGreen ? 47 / 255.0f : 51 / 255.0f;
        g = colour == kRed ? 0.0f : colour == kBlue ? 104 / 255.0f : colour == kGreen ? 221 / 255.0f : 51 / 255.0f;
        b = colour == kRed ? 0.0f : colour == kBlue ? 1.0f : colour == kGreen ? 0.0f : 51 / 255.0f;
      }
#pragma unroll
      for (int j = 0; j < kPix; ++j) {
        const float d = distance<kVmas>(s, shape, px, py[j], P);
        const float w = s.alpha * fminf(fmaxf(0.5f - d * P.inv_h, 0.0f), 1.0f);
        cr[j] += w * (r - cr[j]);
        cg[j] += w * (g - cg[j]);
        cb[j] += w * (b - cb[j]);
      }
    }
    __syncthreads();  // the list and the counts are rewritten by the next chunk
  }

  if (col < P.S) {
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
      const int row = row0 + kRowStep * j;
      if (row < P.S) {
        const uint32_t R = (uint32_t)floorf(255.0f * cr[j] + 0.5f), G = (uint32_t)floorf(255.0f * cg[j] + 0.5f),
                       B = (uint32_t)floorf(255.0f * cb[j] + 0.5f);
        P.out[((int64_t)frame * P.S + row) * P.S + col] = R | (G << 8) | (B << 16) | 0xff000000u;
      }
    }
  }
}

// [lo, hi) byte span of `count` frames of `elems` elements of 4 bytes under the two-level stride
void span(const void* p, int64_t elems, int64_t episodes, int64_t es, int64_t fpe, int64_t ts, uintptr_t* lo,
          uintptr_t* hi) {
  *lo = (uintptr_t)p;
  *hi = (uintptr_t)p + 4 * (uintptr_t)((episodes - 1) * es + (fpe - 1) * ts + elems);
}

// What every render entry decides about the frame counts, strides and grid before it looks at a pointer:
// DGPPO_EINVAL, 1 when there is nothing to draw, else 0 with the tile counts of one frame.
int frame_grid(const dgppo_render_args* a, int64_t* tiles_x, int64_t* tiles_y) {
  if (a->size < 1 || a->size > 32768 || a->n_frames < 0 || a->frames_per_episode < 1) return DGPPO_EINVAL;
  if (a->n_frames == 0) return 1;
  if (a->states_estride < 0 || a->states_tstride < 0 || a->index_estride < 0 || a->index_tstride < 0 ||
      a->obstacles_estride < 0)
    return DGPPO_EINVAL;
  *tiles_x = (a->size + kTileW - 1) / kTileW, *tiles_y = (a->size + kTileH - 1) / kTileH;
  if (a->n_frames * *tiles_x * *tiles_y > 0x7fffffffLL) return DGPPO_EINVAL;
  return 0;
}

}  // namespace
}  // namespace dgppo

extern "C" int dgppo_render_frames(const dgppo_env_cfg* cfg, const dgppo_render_args* a, void* stream) {
  return dgppo_render_frames_field(cfg, a, nullptr, stream);
}

extern "C" int dgppo_render_frames_field(const dgppo_env_cfg* cfg, const dgppo_render_args* a,
                                         const dgppo_render_field* fld, void* stream) {
  using namespace dgppo;
  if (!cfg || !a) return DGPPO_EINVAL;
  if (fld) {
    if (!fld->values || !fld->palette || fld->gx < 2 || fld->gy < 2 || fld->gx > 32768 || fld->gy > 32768)
      return DGPPO_EINVAL;
    if (fld->bands < 2 || fld->bands > DGPPO_RENDER_MAX_BANDS) return DGPPO_EINVAL;
    for (int i = 0; i < 4; ++i)
      if (!isfinite(fld->extent[i])) return DGPPO_EINVAL;
    if (!(fld->extent[1] > fld->extent[0]) || !(fld->extent[3] > fld->extent[2])) return DGPPO_EINVAL;
    if (!isfinite(fld->half_range) || !(fld->half_range > 0.0f)) return DGPPO_EINVAL;
    if (!(fld->alpha >= 0.0f && fld->alpha <= 1.0f) || !isfinite(fld->line_halfwidth) || fld->line_halfwidth < 0.0f)
      return DGPPO_EINVAL;
  }
  if (vmas::is_vmas(cfg)) return DGPPO_EINVAL;  // the VMAS reference renderers are separate code
  if (cfg->engine < DGPPO_ENGINE_LIDAR || cfg->engine > DGPPO_ENGINE_OMNI) return DGPPO_EINVAL;
  const bool mpe = cfg->engine == DGPPO_ENGINE_MPE, omni = cfg->engine == DGPPO_ENGINE_OMNI;
  const int n = cfg->n_agents, O = cfg->n_obs, N = cfg->n_nodes, E = cfg->n_edges, sd = cfg->state_dim;
  const int ng = cfg->n_goals > 0 ? cfg->n_goals : n;
  if (n < 1 || O < 0 || E < 0 || sd < (omni ? 4 : 2) || N < n + ng + 1 || (mpe && N < n + ng + O + 1))
    return DGPPO_EINVAL;
  if (!(cfg->area_size > 0.0f) || !isfinite(cfg->area_size)) return DGPPO_EINVAL;
  int64_t tiles_x = 0, tiles_y = 0;
  if (const int rc = frame_grid(a, &tiles_x, &tiles_y)) return rc < 0 ? rc : 0;
  const bool rects = !mpe && O > 0;
  if (!a->states || !a->out || (E > 0 && (!a->receivers || !a->senders)) || (rects && !a->obstacles))
    return DGPPO_EINVAL;
  const int64_t S = a->size, F = a->n_frames, fpe = a->frames_per_episode;
  const int64_t episodes = (F + fpe - 1) / fpe, fl = F < fpe ? F : fpe;
  {  // `out` must not overlap the bytes an input spans
    const uintptr_t o0 = (uintptr_t)a->out, o1 = o0 + (uintptr_t)(F * S * S * 4);
    uintptr_t lo[6] = {0, 0, 0, 0, 0, 0}, hi[6] = {0, 0, 0, 0, 0, 0};
    span(a->states, (int64_t)N * sd, episodes, a->states_estride, fl, a->states_tstride, &lo[0], &hi[0]);
    if (E > 0) {
      span(a->receivers, E, episodes, a->index_estride, fl, a->index_tstride, &lo[1], &hi[1]);
      span(a->senders, E, episodes, a->index_estride, fl, a->index_tstride, &lo[2], &hi[2]);
    }
    if (rects) span(a->obstacles, (int64_t)O * DGPPO_OBST_FIELDS, episodes, a->obstacles_estride, 1, 0, &lo[3], &hi[3]);
    if (fld) {
      span(fld->values, (int64_t)fld->gx * fld->gy, F, (int64_t)fld->gx * fld->gy, 1, 0, &lo[4], &hi[4]);
      span(fld->palette, 3 * (int64_t)fld->bands, 1, 0, 1, 0, &lo[5], &hi[5]);
    }
    for (int i = 0; i < 6; ++i)
      if (lo[i] < o1 && o0 < hi[i]) return DGPPO_EINVAL;
  }
  Params P{};
  P.states = a->states, P.receivers = a->receivers, P.senders = a->senders, P.obstacles = a->obstacles;
  P.out = (uint32_t*)a->out;
  P.s_es = a->states_estride, P.s_ts = a->states_tstride, P.i_es = a->index_estride, P.i_ts = a->index_tstride;
  P.o_es = a->obstacles_estride;
  P.fpe = (int32_t)fpe, P.S = (int32_t)S, P.tiles_x = (int32_t)tiles_x, P.tiles_per_frame = (int32_t)(tiles_x * tiles_y);
  P.n = n, P.ng = ng, P.O = O, P.N = N, P.E = E, P.sd = sd;
  P.nA = mpe ? O : 0;
  P.nB = omni && (a->flags & DGPPO_RENDER_FOV) ? n - 1 : 0;
  P.nC = E;
  P.nD = ng + n;
  P.nE = rects ? O : 0;
  P.L = cfg->area_size;
  P.h = cfg->area_size / (float)S;
  P.inv_h = 1.0f / P.h;
  P.car_r = cfg->car_radius, P.obs_r = cfg->obs_radius, P.fov_r = cfg->fov_rmax;
  const double beta = (double)cfg->fov_angle_deg * (3.14159265358979323846 / 180.0);
  P.sin_b = (float)sin(beta), P.cos_b = (float)cos(beta);
  P.edge_hw = cfg->area_size / 720.0f;  // the reference's 2 pt line on its 10 in figure
  const dim3 grid((unsigned)(F * tiles_x * tiles_y));
  if (!fld) {
    hipLaunchKernelGGL(render_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, P);
    return (int)hipGetLastError();
  }
  P.field = fld->values, P.palette = fld->palette;
  P.gx = fld->gx, P.gy = fld->gy, P.bands = fld->bands;
  P.fx0 = fld->extent[0], P.fy0 = fld->extent[2];
  P.inv_dx = (float)((double)(fld->gx - 1) / ((double)fld->extent[1] - (double)fld->extent[0]));
  P.inv_dy = (float)((double)(fld->gy - 1) / ((double)fld->extent[3] - (double)fld->extent[2]));
  P.f_half = fld->half_range;
  P.inv_band = (float)((double)fld->bands / (2.0 * (double)fld->half_range));
  P.f_alpha = fld->alpha, P.line_hw = fld->line_halfwidth;
  P.grad_eps = 1e-6f * fld->half_range;
  hipLaunchKernelGGL(render_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, P);
  return (int)hipGetLastError();
}

extern "C" int dgppo_render_frames_vmas(const dgppo_env_cfg* cfg, const dgppo_render_args* a, void* stream) {
  using namespace dgppo;
  if (!cfg || !a) return DGPPO_EINVAL;
  if (!vmas::is_vmas(cfg)) return DGPPO_EINVAL;  // every other engine: dgppo_render_frames
  const bool wheel = cfg->engine == DGPPO_ENGINE_VMAS_WHEEL;
  const int N = cfg->n_nodes, sd = cfg->state_dim;
  if (cfg->n_agents != 3 || N != 4 || sd < 4) return DGPPO_EINVAL;
  if (!(cfg->area_size > 0.0f) || !isfinite(cfg->area_size)) return DGPPO_EINVAL;
  if (a->flags != 0) return DGPPO_EINVAL;
  int64_t tiles_x = 0, tiles_y = 0;
  if (const int rc = frame_grid(a, &tiles_x, &tiles_y)) return rc < 0 ? rc : 0;
  if (!a->states || !a->out || !a->obstacles) return DGPPO_EINVAL;
  const int64_t S = a->size, F = a->n_frames, fpe = a->frames_per_episode;
  const int64_t episodes = (F + fpe - 1) / fpe, fl = F < fpe ? F : fpe;
  {  // `out` must not overlap the bytes an input spans
    const uintptr_t o0 = (uintptr_t)a->out, o1 = o0 + (uintptr_t)(F * S * S * 4);
    uintptr_t lo[2], hi[2];
    span(a->states, (int64_t)N * sd, episodes, a->states_estride, fl, a->states_tstride, &lo[0], &hi[0]);
    span(a->obstacles, DGPPO_VMAS_FIELDS, episodes, a->obstacles_estride, 1, 0, &lo[1], &hi[1]);
    for (int i = 0; i < 2; ++i)
      if (lo[i] < o1 && o0 < hi[i]) return DGPPO_EINVAL;
  }
  Params P{};
  P.states = a->states, P.obstacles = a->obstacles, P.out = (uint32_t*)a->out;
  P.s_es = a->states_estride, P.s_ts = a->states_tstride, P.o_es = a->obstacles_estride;
  P.fpe = (int32_t)fpe, P.S = (int32_t)S, P.tiles_x = (int32_t)tiles_x, P.tiles_per_frame = (int32_t)(tiles_x * tiles_y);
  P.n = 3, P.N = N, P.sd = sd;
  P.wheel = wheel, P.vmas_prims = wheel ? 7 : 10;
  // the view: the reference's set_xlim(-m hw, m hw), m = 1.02 (Wheel) / 1.01 (Transport)
  const float V = (wheel ? 1.02f : 1.01f) * cfg->area_size;
  P.L = cfg->area_size;
  P.half_view = 0.5f * V;
  P.h = V / (float)S;
  P.inv_h = 1.0f / P.h;
  P.car_r = cfg->car_radius;
  P.edge_hw = V / 720.0f;      // the goal ray: a 2 pt line on the 10 in figure
  P.outline_hw = V / 1440.0f;  // a patch's default 1 pt outline
  P.goal_r = cfg->dist2goal, P.box_centre_r = 0.5f * cfg->dist2goal;
  P.fov_r = 1.2f * kLineLength;  // the avoid sector, half-angle 15 degrees (vmas_wheel.py:346-350)
  const double beta = 15.0 * (3.14159265358979323846 / 180.0);
  P.sin_b = (float)sin(beta), P.cos_b = (float)cos(beta);
  hipLaunchKernelGGL((render_kernel<false, true>), dim3((unsigned)(F * tiles_x * tiles_y)), dim3(kThreads), 0,
                     (hipStream_t)stream, P);
  return (int)hipGetLastError();
}
