// Stand-alone host check of pc_crop_metrics_layout (pc_host.cpp: no device, no HIP): sizes,
// offsets and every argument check, meant to be built with the host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/curate_layout_check.cpp person_capture_amd/csrc/pc_host.cpp -o /tmp/curate_layout_check
// The offset array is allocated at exactly n * 5 words, so a write past it is reported.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../include/pcgpu.h"

static int fails = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++fails; } \
  } while (0)

static pc_curate_desc desc(int h, int w) {
  pc_curate_desc d;
  memset(&d, 0, sizeof d);
  d.w = w; d.h = h; d.row_stride = 3 * w;
  const int m = w > h ? w : h;
  d.w2 = w; d.h2 = h;
  d.kind[0] = PC_CURATE_COPY;
  if (m > 256) {
    const double s = 256.0 / (double)m;
    d.w2 = (int)nearbyint(w * s); d.h2 = (int)nearbyint(h * s);
    d.kind[0] = PC_CURATE_AREA;
  }
  d.kind[1] = (w == 32 && h == 32) ? PC_CURATE_COPY : PC_CURATE_AREA;
  return d;
}

int main() {
  const int shapes[][2] = {{33, 47}, {256, 256}, {257, 129}, {32, 32}, {8200, 32}, {32, 8200}, {16384, 16384}, {640, 427}};
  const int n = (int)(sizeof shapes / sizeof shapes[0]);
  std::vector<pc_curate_desc> d;
  for (int i = 0; i < n; ++i) d.push_back(desc(shapes[i][0], shapes[i][1]));
  uint64_t* off = (uint64_t*)malloc(sizeof(uint64_t) * 5 * n);
  size_t sb = 0, ob = 0;
  EXPECT(pc_crop_metrics_layout(d.data(), n, off, &sb, &ob) == PC_OK);
  uint64_t s_end = 0, o_end = ((uint64_t)n * sizeof(pc_curate_record) + 15) & ~15ull;
  for (int i = 0; i < n; ++i) {
    const uint64_t* o = off + 5 * i;
    const uint64_t gp = ((uint64_t)d[i].w + 15) & ~15ull;
    EXPECT(o[0] == s_end && o[0] % 16 == 0);
    s_end += gp * d[i].h;
    if (d[i].kind[0] == PC_CURATE_COPY) EXPECT(o[1] == o[0]);
    else { EXPECT(o[1] == s_end); s_end += (((uint64_t)d[i].w2 + 15) & ~15ull) * d[i].h2; }
    if (d[i].kind[1] == PC_CURATE_COPY) EXPECT(o[2] == o[0]);
    else { EXPECT(o[2] == s_end); s_end += 1024; }
    EXPECT(o[3] == (uint64_t)i * sizeof(pc_curate_record));
    EXPECT(o[4] == o_end && o[4] % 16 == 0);
    o_end += (((uint64_t)d[i].h + d[i].w) * 4 + 15) & ~15ull;
  }
  EXPECT(sb == s_end && ob == o_end);
  // argument checks: nothing is written for a refused batch beyond the images before it
  EXPECT(pc_crop_metrics_layout(nullptr, 1, off, &sb, &ob) == PC_ERR_ARG);
  EXPECT(pc_crop_metrics_layout(d.data(), n, nullptr, &sb, &ob) == PC_ERR_ARG);
  EXPECT(pc_crop_metrics_layout(d.data(), n, off, nullptr, &ob) == PC_ERR_ARG);
  EXPECT(pc_crop_metrics_layout(d.data(), -1, off, &sb, &ob) == PC_ERR_ARG);
  EXPECT(pc_crop_metrics_layout(nullptr, 0, nullptr, &sb, &ob) == PC_OK && sb == 0 && ob == 0);
  struct { int h, w; } bad_size[] = {{31, 40}, {40, 31}, {16385, 40}, {40, 16385}, {16384, 32}, {0, 0}, {-5, 64}};
  for (auto b : bad_size) {
    pc_curate_desc q = desc(b.h > 0 ? b.h : 64, b.w > 0 ? b.w : 64);
    q.h = b.h; q.w = b.w;
    if (b.h == 16384 && b.w == 32) q = desc(16384, 32);   // w2 rounds to 0
    EXPECT(pc_crop_metrics_layout(&q, 1, off, &sb, &ob) == PC_ERR_ARG);
  }
  for (int k = 0; k < 8; ++k) {
    pc_curate_desc q = desc(640, 427);
    if (k == 0) q.w2 += 1;
    if (k == 1) q.h2 -= 1;
    if (k == 2) q.row_stride = 3 * 427 - 1;
    if (k == 3) q.kind[0] = 7;
    if (k == 4) q.kind[1] = PC_CURATE_COPY;
    if (k == 5) { q.kind[0] = PC_CURATE_FAST; q.isx[0] = 3; q.isy[0] = 3; }
    if (k == 6) { q.kind[1] = PC_CURATE_FAST; q.isx[1] = 0; q.isy[1] = 20; }
    if (k == 7) q.xs[0] = -1;
    EXPECT(pc_crop_metrics_layout(&q, 1, off, &sb, &ob) == PC_ERR_ARG);
  }
  free(off);
  printf(fails ? "curate layout check: %d failures\n" : "curate layout check ok\n", fails);
  return fails ? 1 : 0;
}
