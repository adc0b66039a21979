/*
 * sanitize_main.c — drives the oracle under AddressSanitizer + UBSan (TEST INFRASTRUCTURE
 * ONLY: built by `make -C oracle sanitize`, run by tests/test_oracle.py::
 * test_oracle_under_sanitizers).  A separate executable, so the sanitizer runtime is the
 * program's own (no preload into Python).
 *
 * usage: oracle_sanitize <big.nnue> <small.nnue> <fens.txt>
 * For every FEN line: or_eval_fen in the three modes, or_expand_eval and
 * or_expand_eval_inc (BIG mode; their results must agree), or_trace_fen on both nets,
 * and perft(2).  Prints one
 * line per FEN: "<final_v FULL> <final_cp FULL> <n children> <sum of child final_v> <perft2>",
 * or "bad" for a rejected FEN.
 * Then the first PARAM_FENS accepted FENs again under one non-default or_eval_params (PARAMS
 * below: every group of fields moved, a negative rule50 divisor, int32 products that wrap), one
 * line each: "params <index> <final_v> <final_cp> <flags> in modes FULL, BIG, SMALL" (9 numbers),
 * and, back at the defaults, a check that the first FEN evaluates as it did before.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oracle.h"

#define PARAM_FENS 6
static const or_eval_params PARAMS = {700,  2000003, -1999993, 150, 9000, 27000, 400, 700, 50000, -212, 300,
                                      {180, 700, 900, 1400, 2300}, {-20.5, 80.25, -90.125, 300.0625}, 10, 60, 40,
                                      {2, 3, 4, 6, 10}};

int main(int argc, char **argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s big.nnue small.nnue fens.txt\n", argv[0]);
    return 2;
  }
  char err[256];
  or_net *big = NULL, *small = NULL;
  if (or_net_load(argv[1], &big, err, sizeof err) || or_net_load(argv[2], &small, err, sizeof err)) {
    fprintf(stderr, "net: %s\n", err);
    return 2;
  }
  FILE *f = fopen(argv[3], "r");
  if (!f) return 2;
  char line[512];
  or_eval par, par2, *ch = malloc(256 * sizeof(or_eval)), *ch2 = malloc(256 * sizeof(or_eval));
  uint16_t mv[256], mv2[256];
  int rc = 0;
  while (fgets(line, sizeof line, f)) {
    line[strcspn(line, "\r\n")] = 0;
    if (!line[0]) continue;
    or_eval e[3];
    int bad = 0;
    for (int m = 0; m < 3; ++m) bad |= or_eval_fen(big, small, line, m, &e[m]) != 0;
    if (bad) {
      printf("bad\n");
      continue;
    }
    const int n = or_expand_eval(big, small, line, OR_MODE_BIG, &par, mv, ch, 256);
    const int n2 = or_expand_eval_inc(big, small, line, OR_MODE_BIG, &par2, mv2, ch2, 256);
    if (n != n2 || n < 0 || memcmp(&par, &par2, sizeof par) || memcmp(mv, mv2, (size_t)(n > 0 ? n : 0) * 2) ||
        memcmp(ch, ch2, (size_t)(n > 0 ? n : 0) * sizeof(or_eval))) {
      fprintf(stderr, "refresh and incremental expansion differ: %s\n", line);
      rc = 1;
    }
    or_trace tb, ts;
    if (or_trace_fen(big, line, &tb) || or_trace_fen(small, line, &ts) || tb.bucket != ts.bucket) {
      fprintf(stderr, "trace failed: %s\n", line);
      rc = 1;
    }
    long long sum = 0;
    for (int k = 0; k < n; ++k) sum += ch[k].final_v;
    printf("%d %d %d %lld %llu\n", e[0].final_v, e[0].final_cp, n, sum, (unsigned long long)or_perft(line, 2));
  }
  /* the parameterised epilogue */
  rewind(f);
  or_eval_params defaults, back, zero = PARAMS;
  zero.rule50_div = 0;
  or_get_eval_params(&defaults);
  if (or_set_eval_params(&PARAMS)) rc = 1;
  if (or_set_eval_params(&zero) != -1) rc = 1; /* refused: PARAMS stay */
  or_get_eval_params(&back);
  if (memcmp(&back, &PARAMS, sizeof back)) rc = 1;
  for (int i = 0, k = 0; k < PARAM_FENS && fgets(line, sizeof line, f); ++i) {
    line[strcspn(line, "\r\n")] = 0;
    or_eval e[3];
    int bad = !line[0];
    for (int m = 0; m < 3 && !bad; ++m) bad |= or_eval_fen(big, small, line, m, &e[m]) != 0;
    if (bad) continue;
    ++k;
    printf("params %d %d %d %u %d %d %u %d %d %u\n", i, e[0].final_v, e[0].final_cp, (unsigned)e[0].flags,
           e[1].final_v, e[1].final_cp, (unsigned)e[1].flags, e[2].final_v, e[2].final_cp, (unsigned)e[2].flags);
  }
  if (or_set_eval_params(NULL)) rc = 1;
  or_get_eval_params(&back);
  if (memcmp(&back, &defaults, sizeof back)) {
    fprintf(stderr, "defaults not restored\n");
    rc = 1;
  }
  fclose(f);
  free(ch), free(ch2);
  or_net_free(big), or_net_free(small);
  return rc;
}
