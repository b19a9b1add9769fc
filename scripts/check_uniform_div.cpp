// Host evidence for the lookup's short division (csrc/corr_lookup.hip, grid_norm):
// for a divisor s that is the same for a whole workgroup and r = rn(1 / s),
//   q0 = rn(x * r),  e = fma(-q0, s, x),  q = fma(e, r, q0)
// is compared, bit for bit, against the IEEE quotient x / s over all 2^32 float
// bit patterns of x, for every integer divisor 1 ... 511 and a sample of larger
// ones; so is the value the lookup uses, g = q - 1.
//
// Plain C++, explicit fmaf, to be compiled with contraction off:
//   g++ -O3 -march=native -ffp-contract=off -fno-math-errno -pthread
//       scripts/check_uniform_div.cpp -o check_uniform_div
//   ./check_uniform_div [first [last [threads]]]      (default 1 511, all cores)
// Per divisor it prints the exponent range of x (biased, 0 = zero / subnormal,
// 255 = inf / NaN) in which q or g differ; the last lines are the union.  Exit
// status 1 if g differs for any finite x, or q for any x with biased exponent in
// [Q_LO, Q_HI] (the range DESIGN 3.4 quotes).
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace {

constexpr int Q_LO = 127 - 100, Q_HI = 127 + 100;   // 2^-100 <= |x| < 2^101

inline float short_div(float x, float s, float r) {
  const float q0 = x * r;
  const float e = fmaf(-q0, s, x);
  return fmaf(e, r, q0);
}

struct Tally {
  uint64_t q_bad[256] = {}, g_bad[256] = {};   // by biased exponent of x
};

// all mantissas and both signs of one exponent
void run_exponent(float s, float r, int ex, uint64_t& qb, uint64_t& gb) {
  uint64_t nq = 0, ng = 0;
  for (uint32_t sign = 0; sign < 2; ++sign) {
    const uint32_t hi = (sign << 31) | ((uint32_t)ex << 23);
    uint32_t cq = 0, cg = 0;
#pragma GCC ivdep
    for (uint32_t m = 0; m < (1u << 23); ++m) {
      const uint32_t xb = hi | m;
      float x;
      memcpy(&x, &xb, 4);
      const float qa = x / s, qs = short_div(x, s, r);
      const float ga = qa - 1.f, gs = qs - 1.f;
      uint32_t a, b, c, d;
      memcpy(&a, &qa, 4); memcpy(&b, &qs, 4); memcpy(&c, &ga, 4); memcpy(&d, &gs, 4);
      cq += a != b;
      cg += c != d;
    }
    nq += cq; ng += cg;
  }
  qb = nq; gb = ng;
}

void span(const uint64_t* v, int& lo, int& hi, uint64_t& n) {
  lo = 256; hi = -1; n = 0;
  for (int e = 0; e < 256; ++e)
    if (v[e]) { if (e < lo) lo = e; hi = e; n += v[e]; }
}

}  // namespace

int main(int argc, char** argv) {
  const int first = argc > 1 ? atoi(argv[1]) : 1, last = argc > 2 ? atoi(argv[2]) : 511;
  const int nthr = argc > 3 ? atoi(argv[3]) : (int)std::thread::hardware_concurrency();
  std::vector<float> divs;
  for (int d = first; d <= last; ++d) divs.push_back((float)d);
  // large divisors: around powers of two, all-ones significands, ordinary odd values
  for (float d : {513.f, 719.f, 959.f, 1023.f, 1025.f, 1919.f, 2047.f, 4095.f, 8191.f, 65535.f,
                  1048575.f, 16777215.f})
    divs.push_back(d);
  std::vector<Tally> tal(divs.size());
  std::atomic<size_t> next{0};
  std::mutex io;
  auto work = [&] {
    for (size_t i; (i = next.fetch_add(1)) < divs.size();) {
      const float s = divs[i], r = 1.0f / s;
      for (int ex = 0; ex < 256; ++ex) run_exponent(s, r, ex, tal[i].q_bad[ex], tal[i].g_bad[ex]);
      int ql, qh, gl, gh;
      uint64_t nq, ng;
      span(tal[i].q_bad, ql, qh, nq);
      span(tal[i].g_bad, gl, gh, ng);
      std::lock_guard<std::mutex> lk(io);
      if (nq || ng)
        printf("s=%.0f q differs: %llu x, exponents %d..%d; g differs: %llu x, exponents %d..%d\n", s,
               (unsigned long long)nq, ql, qh, (unsigned long long)ng, gl, gh);
      else
        printf("s=%.0f identical for all x\n", s);
      fflush(stdout);
    }
  };
  std::vector<std::thread> th;
  for (int t = 0; t < (nthr > 0 ? nthr : 1); ++t) th.emplace_back(work);
  for (auto& t : th) t.join();

  Tally u;
  for (const Tally& t : tal)
    for (int e = 0; e < 256; ++e) { u.q_bad[e] += t.q_bad[e]; u.g_bad[e] += t.g_bad[e]; }
  int ql, qh, gl, gh;
  uint64_t nq, ng;
  span(u.q_bad, ql, qh, nq);
  span(u.g_bad, gl, gh, ng);
  printf("union over %zu divisors: q differs for %llu x", divs.size(), (unsigned long long)nq);
  if (nq) {
    printf(" at biased exponents");
    for (int e = 0; e < 256; ++e) if (u.q_bad[e]) printf(" %d", e);
  }
  printf("\nunion: g = q - 1 differs for %llu x", (unsigned long long)ng);
  if (ng) {
    printf(" at biased exponents");
    for (int e = 0; e < 256; ++e) if (u.g_bad[e]) printf(" %d", e);
  }
  printf("\n");
  bool fail = false;
  for (int e = 0; e < 255; ++e) fail |= u.g_bad[e] != 0;
  for (int e = Q_LO; e <= Q_HI; ++e) fail |= u.q_bad[e] != 0;
  printf(fail ? "FAIL\n" : "OK: g identical for every finite x; q identical for 2^-100 <= |x| < 2^101\n");
  return fail;
}
