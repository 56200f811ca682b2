// half_l2_bound_model.cpp — the error bound of the half-precision Euclidean selection (velesdb_amd/csrc/vdb_half_l2.hpp, the text the
// library compiles) against f32 accumulations in several orders: half_l2_delta must dominate |s - (|q|^2 - chain) / 2| for s = q.v - h
// with q.v added up sequentially, pairwise and in blocks of 32, h = (f32 norm)^2 / 2 as the kernel takes it, chain = the declared
// 64-lane chain of sweep_half_l2.hip; and half_l2_tau must sit at or under (|q|^2 - chain) / 2 - delta.  Prints one JSON line.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "vdb_half_l2.hpp"

static float bf16_round(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  u &= 0xFFFF0000u;
  memcpy(&x, &u, 4);
  return x;
}
static float f16_round(float x) {  // IEEE f16, round to nearest even (finite range of the data below: no overflow)
  if (fabsf(x) < 6.103515625e-5f) return rintf(x * 16777216.0f) / 16777216.0f;  // subnormals: multiples of 2^-24
  uint32_t u;
  memcpy(&u, &x, 4);
  u += 0xFFFu + ((u >> 13) & 1u);
  u &= 0xFFFFE000u;
  memcpy(&x, &u, 4);
  return x;
}

static float dot_seq(const std::vector<float>& p) {
  float s = 0.f;
  for (float x : p) s += x;
  return s;
}
static float dot_pair(const float* p, size_t n) { return n == 1 ? p[0] : dot_pair(p, n / 2) + dot_pair(p + n / 2, n - n / 2); }
static float dot_blocks(const std::vector<float>& p) {
  float s = 0.f;
  for (size_t b = 0; b < p.size(); b += 32) s += dot_pair(p.data() + b, 32);
  return s;
}
// the declared chain: chunk c = i / 8 belongs to lane c % 64, one fmaf chain per lane, xor butterfly 32 .. 1
static float chain(const std::vector<float>& q, const std::vector<float>& v) {
  float t[64] = {0};
  for (size_t i = 0; i < q.size(); i++) {
    const float d = q[i] - v[i];
    float& a = t[(i / 8) % 64];
    a = fmaf(d, d, a);
  }
  for (int s = 32; s >= 1; s >>= 1) {
    float u[64];
    for (int l = 0; l < 64; l++) u[l] = t[l] + t[l ^ s];
    memcpy(t, u, sizeof t);
  }
  return t[0];
}

int main() {
  std::mt19937 rng(5);
  std::normal_distribution<float> nd(0.f, 1.f);
  int failed = 0, cases = 0;
  double worst = 0.0;
  for (uint32_t dim : {128u, 192u, 768u, 2048u, 4096u})
    for (int f16 = 0; f16 < 2; f16++)
      for (int kind = 0; kind < 3; kind++)  // N(0,1); large norms; a near-duplicate of the query
        for (int rep = 0; rep < 40; rep++) {
          const float scale = kind == 1 ? (f16 ? 40.f : 1e4f) : 1.f;
          std::vector<float> q(dim), v(dim), p(dim);
          double qn2 = 0, vn2 = 0;
          float nsq = 0.f;
          for (uint32_t i = 0; i < dim; i++) {
            const float a = nd(rng) * scale, b = kind == 2 ? a + 1e-3f * nd(rng) : nd(rng) * scale;
            q[i] = f16 ? f16_round(a) : bf16_round(a);
            v[i] = f16 ? f16_round(b) : bf16_round(b);
            p[i] = q[i] * v[i];  // exact in f32
            qn2 += (double)q[i] * q[i];
            vn2 += (double)v[i] * v[i];
            nsq = fmaf(v[i], v[i], nsq);
          }
          const float nrm = sqrtf(nsq), h = 0.5f * nrm * nrm;
          const float ch = chain(q, v);
          const double want = 0.5 * (qn2 - (double)ch);
          const double vmax2 = (double)nrm * nrm * (1.0 + 4.76837158203125e-7);
          const double delta = vdb::half_l2_delta(dim, qn2, vmax2, (double)ch);
          for (float dot : {dot_seq(p), dot_pair(p.data(), dim), dot_blocks(p)}) {
            const double err = fabs((double)(dot - h) - want);
            cases++;
            if (!(err <= delta)) failed++;
            if (delta > 0 && err / delta > worst) worst = err / delta;
          }
          // the bound the kernel compares with never exceeds the real one (rounded down), and is within 2^-21 of it
          const double t = want - delta;
          const float tau = vdb::half_l2_tau(dim, qn2, vmax2, (double)ch);
          if (!((double)tau <= t) || !(t - (double)tau <= fabs(t) * 4.8e-7 + 1e-30)) failed++;
          (void)vn2;
        }
  if (!vdb::half_l2_lists_fit(65536 + 77, 128) || !vdb::half_l2_lists_fit(1u << 20, 32) || vdb::half_l2_lists_fit(1u << 20, 33)) failed++;
  printf("{\"cases\": %d, \"failed_checks\": %d, \"worst_err_over_delta\": %.4f}\n", cases, failed, worst);
  return failed ? 1 : 0;
}
