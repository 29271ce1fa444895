// Stand-alone host check of the grouped weight-gradient planner (csrc/gemm.hip: grouped_plan, grouped_plan_ragged),
// meant for host sanitizers -- nothing here touches a GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         tools/grouped_plan_check.hip -Lfocused-attention-vit_amd/lib -lfavit -Wl,-rpath,$PWD/focused-attention-vit_amd/lib \
//         -o tools/probe_build/grouped_plan_check && tools/probe_build/grouped_plan_check
// (libfavit.so only supplies what gemm.hip takes from the other sources; the planner under test is compiled HERE, with
// the sanitizer.)  Over random ragged groups it checks that every (chunk, split) unit sits in exactly one queue, that a
// chunk's k-ranges tile [0, K) with no empty split, and that the workspace query equals what the plan's slabs take.
#include "../focused-attention-vit_amd/csrc/gemm.hip"

#include <stdio.h>
#include <stdlib.h>

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd(unsigned n) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (unsigned)(rng_state % n);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s (line %d, group %d)\n", #c, __LINE__, iter); return 1; } } while (0)

int main() {
  static const long shapes[2][4][2] = {{{384, 1536}, {1536, 384}, {384, 384}, {1152, 384}}, {{384, 128}, {128, 128}, {512, 128}, {128, 512}}};
  favit_gemm_t gs[GROUP_MAX];
  int64_t out[1024];
  for (int iter = 0; iter < 2000; ++iter) {
    const int nblocks = 1 + (int)rnd(12), d = (int)rnd(2);
    static const unsigned spans[3] = {8, 60, 700};
    memset(gs, 0, sizeof(gs));
    for (int b = 0; b < nblocks; ++b) {
      const long T = 32 * (1 + (long)rnd(spans[rnd(3)]));
      for (int j = 0; j < 4; ++j) { gs[4 * b + j].M = shapes[d][j][0]; gs[4 * b + j].N = shapes[d][j][1]; gs[4 * b + j].K = T; }
    }
    const int count = 4 * nblocks;
    const int n = favit_gemm_grouped_plan(gs, count, 1, out, 1024);
    CHECK(n > 0);
    const int nchunks = (int)out[0], nunits = (int)out[1];
    CHECK(nchunks >= 1 && nchunks <= GROUP_MAX && nunits <= 255);
    int units = 0;
    long ws = 0;
    for (int c = 0; c < nchunks; ++c) {
      const int64_t* ch = out + 4 + 5 * c;
      const long first = ch[0], K = ch[2], s = ch[3], kps = ch[4];
      const long last = c + 1 < nchunks ? out[4 + 5 * (c + 1)] : count;
      CHECK(kps > 0 && kps % 32 == 0 && (s - 1) * kps < K && K <= s * kps);
      long fl = 0;
      for (long i = first; i < last; ++i) { CHECK(gs[i].K == K); fl += gs[i].M * gs[i].N + (gs[i].M + 3) / 4 * 4; }
      if (s > 1) ws += s * ((fl + 63) / 64 * 64) * 4;
      units += (int)s;
    }
    CHECK(units == nunits);
    int seen[256] = {0};
    int o = 4 + 5 * nchunks;
    for (int x = 0; x < 8; ++x) {
      const int q = (int)out[o++];
      CHECK(q <= GROUP_XCD_UNITS);
      for (int j = 0; j < q; ++j) { const int u = (int)out[o++]; CHECK(u >= 0 && u < nunits); ++seen[u]; }
    }
    CHECK(o == n);
    for (int u = 0; u < nunits; ++u) CHECK(seen[u] == 1);
    CHECK(out[3] == ws && favit_gemm_grouped_tn_ragged_workspace(gs, count) == ws);
  }
  printf("grouped_plan_check: 2000 random ragged groups ok\n");
  return 0;
}
