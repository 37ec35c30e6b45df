// CPU harness (tests only): the product's half-size scalar search
// (firedancer_amd/csrc/fd25519_half.h) compiled for the host, over a whole
// batch of k at once.  As a shared object it gives tests/test_half_euclid.py
// half_scalars_batch; with -DHALF_EUCLID_MAIN it is a program of its own
// (built with the sanitizers there) that reads a file of k and expected
// results and compares.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// The header's test hooks: every full step that a round accepts from leading
// bits is redone here on the whole integers, with integer arithmetic only.
// From (a, b) at the round's start, a step with quotient q is a true
// Euclidean step iff 0 <= a - q b < b; then (a, b) <- (b, a - q b).
static uint32_t hook_a[8], hook_b[8];
static uint64_t hook_steps, hook_bad;

static void hook_round(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  for (int i = 0; i < 8; i++) { hook_a[i] = a[i]; hook_b[i] = b[i]; }
}

static void hook_step(double qd) {
  hook_steps++;
  if (!(qd >= 1.0 && qd < 0x1p53)) { hook_bad++; return; }
  const uint64_t q = (uint64_t)qd;
  // p = q b over 10 words, r = a - p
  uint32_t p[10], r[8];
  unsigned __int128 c = 0;
  for (int i = 0; i < 8; i++) {
    c += (unsigned __int128)q * hook_b[i];
    p[i] = (uint32_t)c;
    c >>= 32;
  }
  p[8] = (uint32_t)c;
  p[9] = (uint32_t)(c >> 32);
  int64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const int64_t t = (int64_t)hook_a[i] - (int64_t)p[i] - br;
    r[i] = (uint32_t)t;
    br = t < 0;
  }
  int lt = 0;   // r < b
  for (int i = 0; i < 8; i++) lt = r[i] != hook_b[i] ? (r[i] < hook_b[i]) : lt;
  if (br || p[8] || p[9] || !lt) { hook_bad++; return; }
  for (int i = 0; i < 8; i++) { hook_a[i] = hook_b[i]; hook_b[i] = r[i]; }
}

#define FD_HALF_HOOK_ROUND(a, b) hook_round((a), (b))
#define FD_HALF_HOOK_STEP(q) hook_step((q))
#include "fd25519_half.h"

// steps checked and steps that were not true Euclidean steps, since the start
extern "C" void half_hook_counts(uint64_t* steps, uint64_t* bad) {
  *steps = hook_steps;
  *bad = hook_bad;
}

// out: 12 words per k -- found, d < 0, c[5], |d|[5]
extern "C" void half_scalars_batch(const uint32_t* k, uint64_t n, int dbits, uint32_t* out) {
  for (uint64_t i = 0; i < n; i++) {
    uint32_t kk[8], cc[FD_HALF_TW], dd[FD_HALF_TW];
    for (int w = 0; w < 8; w++) kk[w] = k[8 * i + w];
    int neg = 0;
    const int ok = fd_half_scalars(kk, cc, dd, &neg, dbits);
    uint32_t* o = out + 12 * i;
    o[0] = (uint32_t)ok;
    o[1] = (uint32_t)neg;
    for (int w = 0; w < FD_HALF_TW; w++) { o[2 + w] = cc[w]; o[7 + w] = dd[w]; }
  }
}

#ifdef HALF_EUCLID_MAIN
// file: uint64 n, int32 dbits, int32 pad, then n records of 8 words k and
// the 12 expected words; c, |d| and the sign are compared where found is set
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n = 0;
  int32_t hdr[2] = {0, 0};
  if (fread(&n, 8, 1, f) != 1 || fread(hdr, 4, 2, f) != 2) return 2;
  uint32_t* rec = (uint32_t*)malloc(n * 20 * sizeof(uint32_t));
  if (!rec || fread(rec, 20 * sizeof(uint32_t), n, f) != n) return 2;
  fclose(f);
  uint64_t bad = 0;
  for (uint64_t i = 0; i < n; i++) {
    uint32_t got[12];
    half_scalars_batch(rec + 20 * i, 1, hdr[0], got);
    const uint32_t* want = rec + 20 * i + 8;
    if (got[0] != want[0] || (got[0] && memcmp(got, want, sizeof got))) {
      if (bad++ < 8) fprintf(stderr, "record %llu differs (found %u, expected %u)\n", (unsigned long long)i, got[0], want[0]);
    }
  }
  free(rec);
  printf("%llu records, %llu differ, %llu steps, %llu not Euclidean\n", (unsigned long long)n, (unsigned long long)bad,
         (unsigned long long)hook_steps, (unsigned long long)hook_bad);
  return bad || hook_bad ? 1 : 0;
}
#endif
