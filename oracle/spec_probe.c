/* oracle/spec_probe.c -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU model of what cmx_mixnet_spec_kernel's helper workgroups do with one layer-0 dot product (cmix_amd/csrc/mixnet_chunk.hip,
 * helper_role): the 2078 rounded products are cut at 512, 1024 and 1536; the wave of segment q = 1..3 centres 64 candidate
 * starts on an f64 estimate of the f32 running sum at its first term and later either takes the lane whose candidate has the
 * true start's bit pattern or re-runs the segment from the true start. The model restates, operation for operation,
 *   - the estimate: per lane ds += (double)p over k = 0..7 (element 512 q + 64 k + lane), wave_sum_f64's tree in its written
 *     order, then est = 0.0; est += segsum[q'] for q' = 0..q-1, rounded to f32;
 *   - the candidates: ord2f(f2ord((float)est) + lane - 32), matched by bit pattern;
 * and reports which path every speculative segment takes. It changes nothing in the oracle's arithmetic: it is fed through
 * orc_mix_probe (mixnet_oracle.c) or directly with a vector of products (tests/spec_model.py).
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define SPEC_IN0 2078
#define SPEC_SEG 512

typedef struct {
  int64_t offset[3];    /* f2ord(true start) - f2ord((float)est) of segment 1..3; a hit: -32 <= offset <= 31, through lane offset + 32 */
  uint32_t start[3];    /* bit pattern of the true start: the sequential f32 sum of products [0, 512 q) */
  uint32_t centre[3];   /* bit pattern of (float)est */
  uint32_t resolved[3]; /* the running sum after segment q as the kernel resolves it: run from the hit lane's candidate, or re-run from the true start */
  uint32_t serial[3];   /* the same run from the true start (what the reference computes) */
  uint32_t sum;         /* the whole chain */
  uint32_t pad;
} orc_spec_rec;

/* the mixing network's hook (mixnet_oracle.c), declared here so that this file needs nothing of the other oracle sources */
extern void (*orc_mix_probe)(const void* mixer, const float* in, const float* w, int n_in);

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
/* the kernel's f2ord / ord2f: float <-> integer of the same order; -0.0 -> -1, +0.0 -> 0 */
static int32_t f2ord(float f) { int32_t b = (int32_t)bits_of(f); return b ^ ((b >> 31) & 0x7fffffff); }
static float ord2f(int32_t o) { return float_of((uint32_t)(o ^ ((o >> 31) & 0x7fffffff))); }

static float seg_run(float s, const float* x, int n) {
  for (int i = 0; i < n; ++i) s += x[i];
  return s;
}

/* wave_sum_f64 as lane 0, 16, 32, 48 see it: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_ror:4, row_ror:8 (lane i of a row of 16
 * reads lane (i - n) mod 16), then (lane 0 + lane 16) + (lane 32 + lane 48) */
static double wave_sum(const double v[64]) {
  double r[4];
  for (int row = 0; row < 4; ++row) {
    double q[4];
    for (int j = 0; j < 4; ++j) {
      const double* p = v + 16 * row + 4 * j;
      q[j] = (p[0] + p[1]) + (p[2] + p[3]);
    }
    const double a0 = q[0] + q[3]; /* lane 0 after row_ror:4 (reads lane 12) */
    const double a8 = q[2] + q[1]; /* lane 8 after row_ror:4 (reads lane 4) */
    r[row] = a0 + a8;              /* lane 0 after row_ror:8 (reads lane 8) */
  }
  return (r[0] + r[1]) + (r[2] + r[3]);
}

void orc_spec_model(const float* prod, orc_spec_rec* out) {
  double segsum[3];
  for (int q = 0; q < 3; ++q) {
    double v[64];
    for (int lane = 0; lane < 64; ++lane) {
      double ds = 0.0;
      for (int k = 0; k < 8; ++k) ds += (double)prod[SPEC_SEG * q + 64 * k + lane];
      v[lane] = ds;
    }
    segsum[q] = wave_sum(v);
  }
  memset(out, 0, sizeof *out);
  float s = seg_run(0.0f, prod, SPEC_SEG);
  for (int w = 1; w <= 3; ++w) {
    const int n = w == 3 ? SPEC_IN0 - 3 * SPEC_SEG : SPEC_SEG;
    double est = 0.0;
    for (int q = 0; q < w; ++q) est += segsum[q];
    const float centre = (float)est;
    const int64_t off = (int64_t)f2ord(s) - (int64_t)f2ord(centre);
    const float serial = seg_run(s, prod + SPEC_SEG * w, n);
    float resolved = serial;
    if (off >= -32 && off <= 31) resolved = seg_run(ord2f(f2ord(centre) + (int32_t)off), prod + SPEC_SEG * w, n);
    out->offset[w - 1] = off;
    out->start[w - 1] = bits_of(s);
    out->centre[w - 1] = bits_of(centre);
    out->resolved[w - 1] = bits_of(resolved);
    out->serial[w - 1] = bits_of(serial);
    s = serial;
  }
  out->sum = bits_of(s);
}

/* recorder: one record per layer-0 Mix, in call order (bit-major, mixer 0..25 within a bit) */
static orc_spec_rec* g_buf;
static size_t g_cap, g_n;

static void spec_probe(const void* mixer, const float* in, const float* w, int n_in) {
  (void)mixer;
  if (n_in != SPEC_IN0) return;
  static float x[SPEC_IN0];
  for (int i = 0; i < n_in; ++i) x[i] = in[i] * w[i]; /* mixer.cpp:41: the product rounded to float (this file is built with -ffp-contract=off) */
  if (g_n < g_cap) orc_spec_model(x, g_buf + g_n);
  ++g_n;
}

void orc_spec_record_begin(orc_spec_rec* buf, size_t cap) {
  g_buf = buf; g_cap = cap; g_n = 0;
  orc_mix_probe = spec_probe;
}

/* returns the number of layer-0 mixes seen since orc_spec_record_begin (more than cap: the buffer was too small) */
size_t orc_spec_record_end(void) {
  orc_mix_probe = 0;
  g_buf = 0; g_cap = 0;
  return g_n;
}
