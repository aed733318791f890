"""The drop-in boundary exercised the way a foreign-language host would: a plain C99 program (no Python, no torch) creates
a context, runs lemsm_msm / lemsm_lhs_msm on the committed golden vectors and compares the canonical bytes; and the
host-side challenge helpers of SURVEY 8(f).4 re-run under the gpu marker so that the driver's GPU record covers them."""
import json
import os
import subprocess

import numpy as np
import pytest

from helpers import golden_points_raw, golden_scalars, jacobian_with_random_z
from halo2_liam_eagen_msm_amd import _lib
from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

C_SRC = r'''
#include "lemsm.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
/* file: u32 kind (0 msm, 1 lhs), u32 curve, u32 n, u32 base, then n x 32 B scalars, n x (kind ? 96 : 64) B points, 64 B expected */
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
  unsigned hdr[4]; if (fread(hdr, 4, 4, f) != 4) return 4;
  const unsigned kind = hdr[0], curve = hdr[1], n = hdr[2], base = hdr[3];
  const size_t pb = kind ? 96 : 64;
  uint8_t* sc = malloc((size_t)n * 32 + 1); uint64_t* pts = malloc((size_t)n * pb + 8); uint8_t want[64], got[64];
  if (fread(sc, 32, n, f) != n || fread(pts, pb, n, f) != n || fread(want, 1, 64, f) != 64) return 5;
  fclose(f);
  lemsm_ctx* ctx = NULL;
  int rc = lemsm_create(0, &ctx); if (rc != LEMSM_OK) { fprintf(stderr, "create: %s\n", lemsm_strerror(rc)); return 6; }
  uint64_t out[12];
  if (kind == 0) rc = lemsm_msm(ctx, (int)curve, sc, pts, n, out);
  else rc = lemsm_lhs_msm(ctx, (int)curve, sc, pts, n, (uint8_t)base, out, NULL, NULL);
  if (rc != LEMSM_OK) { fprintf(stderr, "call: %s (%s)\n", lemsm_strerror(rc), lemsm_last_error(ctx)); return 7; }
  if (lemsm_jacobian_to_canonical((int)curve, out, got) != LEMSM_OK) return 8;
  lemsm_destroy(ctx);
  if (memcmp(got, want, 64) != 0) { fprintf(stderr, "mismatch\n"); return 9; }
  printf("OK %u %u %u\n", kind, curve, n);
  free(sc); free(pts);
  return 0;
}
'''


def _build(tmp_path):
    src = tmp_path / "c_host.c"
    src.write_text(C_SRC)
    exe = tmp_path / "c_host"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-llemsm", "-Wl,-rpath," + libdir])
    return exe


def test_c_program_runs_the_golden_vectors(tmp_path):
    exe = _build(tmp_path)
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "msm_vectors.json")))
    ran = 0
    for v in vec["msm"]:
        c = pyref.CURVES[v["curve"]]
        sc = golden_scalars(v["scalars"]); pts = golden_points_raw(c, v["points"])
        f = tmp_path / ("msm_%d.bin" % ran)
        with open(f, "wb") as fh:
            fh.write(np.array([0, c.cid, sc.shape[0], 0], np.uint32).tobytes()); fh.write(np.ascontiguousarray(sc).tobytes())
            fh.write(np.ascontiguousarray(pts, np.uint64).tobytes()); fh.write(bytes.fromhex(v["expected"]))
        out = subprocess.check_output([str(exe), str(f)], timeout=120).decode()
        assert out.startswith("OK 0"), out
        ran += 1
    for v in vec["lhs"]:
        c = pyref.CURVES[v["curve"]]
        sc = golden_scalars(v["scalars"]); pts = jacobian_with_random_z(c, golden_points_raw(c, v["points"]), v["seed"])
        f = tmp_path / ("lhs_%d.bin" % ran)
        with open(f, "wb") as fh:
            fh.write(np.array([1, c.cid, sc.shape[0], v["base"]], np.uint32).tobytes()); fh.write(np.ascontiguousarray(sc).tobytes())
            fh.write(np.ascontiguousarray(pts, np.uint64).tobytes()); fh.write(bytes.fromhex(v["expected_carry"]))
        out = subprocess.check_output([str(exe), str(f)], timeout=120).decode()
        assert out.startswith("OK 1"), out
        ran += 1
    assert ran >= 4


# The threading contract of include/lemsm.h from C: two pthreads, a context each on device 0, no Python and no GIL.  Thread 0
# runs the files of kind 0 (msm), thread 1 those of kind 1 (lhs), ROUNDS rounds each, both leaving a barrier together; every
# call's canonical bytes are compared with the file's expected value.  Same file format as the program above.
C_THREADS_SRC = r'''
#define _POSIX_C_SOURCE 200809L
#include "lemsm.h"
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#define ROUNDS 25
#define MAXV 64
typedef struct { unsigned kind, curve, n, base; uint8_t* sc; uint64_t* pts; uint8_t want[64]; } vec_t;
typedef struct { int id; int nv; vec_t* v[MAXV]; int rounds; int rc; char msg[256]; } job_t;
static pthread_barrier_t start;
static int load(const char* path, vec_t* v) {
  FILE* f = fopen(path, "rb"); if (!f) return 3;
  unsigned hdr[4]; if (fread(hdr, 4, 4, f) != 4) { fclose(f); return 4; }
  v->kind = hdr[0]; v->curve = hdr[1]; v->n = hdr[2]; v->base = hdr[3];
  const size_t pb = v->kind ? 96 : 64;
  v->sc = malloc((size_t)v->n * 32 + 1); v->pts = malloc((size_t)v->n * pb + 8);
  if (!v->sc || !v->pts) { fclose(f); return 5; }
  if (fread(v->sc, 32, v->n, f) != v->n || fread(v->pts, pb, v->n, f) != v->n || fread(v->want, 1, 64, f) != 64) { fclose(f); return 5; }
  fclose(f);
  return 0;
}
static void* run(void* arg) {
  job_t* j = arg;
  lemsm_ctx* ctx = NULL;
  int rc = lemsm_create(0, &ctx);
  if (rc != LEMSM_OK) { j->rc = 6; snprintf(j->msg, sizeof j->msg, "create: %s", lemsm_strerror(rc)); }
  pthread_barrier_wait(&start);                 /* (reached on failure too: the other thread must not wait for ever) */
  if (j->rc) return NULL;
  for (int r = 0; r < ROUNDS && !j->rc; r++) {
    for (int k = 0; k < j->nv && !j->rc; k++) {
      const vec_t* v = j->v[k];
      uint64_t out[12]; uint8_t got[64];
      if (v->kind == 0) rc = lemsm_msm(ctx, (int)v->curve, v->sc, v->pts, v->n, out);
      else rc = lemsm_lhs_msm(ctx, (int)v->curve, v->sc, v->pts, v->n, (uint8_t)v->base, out, NULL, NULL);
      if (rc != LEMSM_OK) { j->rc = 7; snprintf(j->msg, sizeof j->msg, "round %d vector %d: %s (%s)", r, k, lemsm_strerror(rc), lemsm_last_error(ctx)); break; }
      if (lemsm_jacobian_to_canonical((int)v->curve, out, got) != LEMSM_OK) { j->rc = 8; snprintf(j->msg, sizeof j->msg, "round %d vector %d: canonical", r, k); break; }
      if (memcmp(got, v->want, 64) != 0) { j->rc = 9; snprintf(j->msg, sizeof j->msg, "round %d vector %d: mismatch", r, k); break; }
    }
    if (!j->rc) j->rounds++;
  }
  lemsm_destroy(ctx);
  return NULL;
}
int main(int argc, char** argv) {
  static vec_t vecs[MAXV];
  static job_t jobs[2];
  if (argc < 3 || argc - 1 > MAXV) return 2;
  for (int i = 1; i < argc; i++) {
    int rc = load(argv[i], &vecs[i - 1]); if (rc) return rc;
    if (vecs[i - 1].kind > 1) return 2;
    job_t* j = &jobs[vecs[i - 1].kind]; j->v[j->nv++] = &vecs[i - 1];
  }
  if (!jobs[0].nv || !jobs[1].nv) return 2;
  if (pthread_barrier_init(&start, NULL, 2)) return 10;
  pthread_t th[2];
  for (int t = 0; t < 2; t++) { jobs[t].id = t; if (pthread_create(&th[t], NULL, run, &jobs[t])) return 10; }
  for (int t = 0; t < 2; t++) pthread_join(th[t], NULL);
  int bad = 0;
  for (int t = 0; t < 2; t++) {
    if (jobs[t].rc) { fprintf(stderr, "thread %d: %s\n", t, jobs[t].msg); bad = jobs[t].rc; }
    else printf("OK thread %d rounds %d vectors %d\n", t, jobs[t].rounds, jobs[t].nv);
  }
  return bad;
}
'''


def _build_threads(tmp_path):
    src = tmp_path / "c_threads.c"
    src.write_text(C_THREADS_SRC)
    exe = tmp_path / "c_threads"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-llemsm", "-Wl,-rpath," + libdir])
    return exe


def _write_msm_file(path, v):
    c = pyref.CURVES[v["curve"]]
    sc = golden_scalars(v["scalars"]); pts = golden_points_raw(c, v["points"])
    with open(path, "wb") as fh:
        fh.write(np.array([0, c.cid, sc.shape[0], 0], np.uint32).tobytes()); fh.write(np.ascontiguousarray(sc).tobytes())
        fh.write(np.ascontiguousarray(pts, np.uint64).tobytes()); fh.write(bytes.fromhex(v["expected"]))


def _write_lhs_file(path, v):
    c = pyref.CURVES[v["curve"]]
    sc = golden_scalars(v["scalars"]); pts = jacobian_with_random_z(c, golden_points_raw(c, v["points"]), v["seed"])
    with open(path, "wb") as fh:
        fh.write(np.array([1, c.cid, sc.shape[0], v["base"]], np.uint32).tobytes()); fh.write(np.ascontiguousarray(sc).tobytes())
        fh.write(np.ascontiguousarray(pts, np.uint64).tobytes()); fh.write(bytes.fromhex(v["expected_carry"]))


def test_c_program_two_pthreads_two_contexts(tmp_path):
    """two pthreads of a plain C99 program, a context each on device 0: thread 0 runs the golden msm vectors, thread 1 the
    golden lhs vectors, 25 rounds each from a common barrier, every result compared as canonical bytes"""
    exe = _build_threads(tmp_path)
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "msm_vectors.json")))
    files = []
    for i, v in enumerate(vec["msm"]):
        files.append(tmp_path / ("msm_%d.bin" % i)); _write_msm_file(files[-1], v)
    for i, v in enumerate(vec["lhs"]):
        files.append(tmp_path / ("lhs_%d.bin" % i)); _write_lhs_file(files[-1], v)
    r = subprocess.run([str(exe)] + [str(f) for f in files], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "OK thread 0 rounds 25 vectors %d" % len(vec["msm"]) in lines, r.stdout + r.stderr
    assert "OK thread 1 rounds 25 vectors %d" % len(vec["lhs"]) in lines, r.stdout + r.stderr


@pytest.mark.parametrize("curve", pyref.CURVES.values(), ids=lambda c: c.name)
def test_challenge_helpers_under_the_gpu_marker(curve):
    """to_curve_x / y_from_x / slope (src/config.rs:166-187) are host functions of the library; this is
    tests/test_host_logic.py's check run again where the driver records it"""
    from test_host_logic import test_to_curve_x_y_from_x_slope
    test_to_curve_x_y_from_x_slope(curve)
