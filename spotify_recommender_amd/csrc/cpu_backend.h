// cpu_backend.h — the product's own CPU backend, for hosts WITHOUT a HIP device.
//
// The reference degrades to a CPU loop when it finds no GPU ("No CUDA devices found. Falling back to CPU",
// Recommender.cu:117-127,176-181) and answers with calculateSimilaritiesCPU (:256-273) + the host heap of
// recommendByIndex (:293-315).  BASELINE configs[0] ("114 k tracks, CPU/OpenMP cosine path only") is that path.
// This file is its counterpart behind mi355rec_create_sharded / mi355rec_create_placed: the same arithmetic —
// strictly sequential j = 0..11, multiply and add rounded separately, IEEE sqrt and divide, `> 1e-8f` on
// sqrt(norm) * qnorm, the std::min / std::max clamp — over the dense row-major matrix, rows split over OpenMP
// threads with a top-N per thread and one merge.  Results are in the engine's canonical order (score descending,
// row ascending; -0.0f ranks and reports as +0.0f), so a caller cannot tell the backends apart by their answers.
//
// It is taken ONLY when hipGetDeviceCount reports no device at all: a host with a GPU never lands here, the
// single-device C-ABI (mi355rec_create) keeps failing with MI355REC_ERR_NO_DEVICE, and nothing under oracle/
// (test infrastructure) is included, linked or loaded by it.  Compiled by g++ with -O3 -ffp-contract=off and
// without -ffast-math / -march (the reference's own flags, Makefile:9): the sums stay unfused and in order.
#pragma once

#include <cstdint>

#include "mi355rec_diag.h"
#include "playlist_request.h"

namespace mi355cpu {

struct Catalogue;

// Copies the n x 12 row-major matrix (the reference deep-copies its songs as well, Recommender.cu:109).
// threads = 0: what OpenMP would use (OMP_NUM_THREADS, else every core the process may run on).
Catalogue* create(const float* feats_rowmajor, int64_t n, int threads);
void destroy(Catalogue* c);
int64_t rows(const Catalogue* c);
int threads(const Catalogue* c);
const float* row(const Catalogue* c, int64_t r);

// calculateSimilaritiesCPU (Recommender.cu:256-273): out_n[i] = cosine(q12, row i).
void scores(const Catalogue* c, const float* q12, float* out_n);

// recommendByIndex's selection (Recommender.cu:293-315) in canonical order: the best min(topn, rows - [exclude is
// a row]) rows, `exclude` (-1: none) skipped by INDEX.  Returns how many were written.
int topn(const Catalogue* c, const float* q12, int64_t exclude, int topn, int64_t* out_idx, float* out_score);

}  // namespace mi355cpu

// ---- the whole "sharded" handle on a host without a device --------------------------------------------------------
// What mi355rec_create_sharded / _placed return there: the synchronous calls and the ticketed stream of
// include/mi355rec.h ("row-sharded catalogue"), served by the catalogue above.  The stream keeps the GPU path's
// bookkeeping — tickets, windows, a ring of 4 windows of results, flushes that round the next ticket up to a window
// boundary — so that a serving loop written against the C-ABI runs unchanged; a query is simply computed when it is
// enqueued.  Return values are the C-ABI's codes (0 = ok, MI355REC_ERR_INVALID_ARG); *why receives a message.
namespace mi355cpu {

struct Node;
Node* node_create(const float* feats_rowmajor, int64_t n);
void node_destroy(Node* h);
const Catalogue* node_catalogue(const Node* h);
int node_query(Node* h, const float* q12, int64_t exclude, int topn, int64_t* out_idx, float* out_score, int* out_count,
               const char** why);
// LABELS (include/mi355rec_diag.h): one label per row (-1 = unlabelled; labels = null drops them), and the query over the
// rows whose label is in set[0..n_set) — the same loop with a label test, the same canonical order.
int node_set_labels(Node* h, const int32_t* labels, int64_t n, const char** why);
int node_query_labels(Node* h, const float* q12, int64_t exclude, const int32_t* set, int n_set, int topn, int64_t* out_idx,
                      float* out_score, int* out_count, const char** why);
// PLAYLISTS (include/mi355rec_diag.h): the top-N rows by the mean of their scores against r.members[0..k) (k x 12, by value:
// the caller has resolved rows), the rows of r.exclude[0..n_exclude) (global ids) left out; r.filter: null, or a feature filter
// ("FEATURE FILTERS") that every returned row passes; r.weights: null (the plain mean), or k signed weights ("WEIGHTED
// PLAYLISTS": score = fl(sum_k fl(w_k c_k)) / fl(sum_k |w_k|)).  The request has been checked by the caller
// (playlist_request.h); the diversified fields are not read.
int node_query_mean(Node* h, const mi355playlist::Request& r, const mi355playlist::Outputs& out, const char** why);
// CANDIDATE SCORES (include/mi355rec_diag.h): the value of every listed row under the same request (members by value, checked; r.listed
// with checked ids), in list order, by node_query_mean's own arithmetic.
int node_score_rows(Node* h, const mi355playlist::Request& r, const mi355playlist::ScoreOutputs& out, const char** why);
// DIVERSIFIED TOP-N (include/mi355rec_diag.h): the top-`pool` of node_query_mean re-ranked by maximal marginal relevance.
// out.score and out.mmr may be null.
int node_query_mean_diverse(Node* h, const mi355playlist::Request& r, const mi355playlist::Outputs& out, const char** why);
// GROUP CAPS (include/mi355rec_diag.h): one group id per row (>= 0, or -1 = never capped; null drops them).  A capped
// request makes node_query_mean_diverse the capped call: a row is eligible while fewer than max_per_group picked
// rows share its group; the loop ends when nothing is eligible; *out_pool_rows = P'.
int node_set_groups(Node* h, const int32_t* groups, int64_t n, const char** why);
// ROW PRIORS: one fp32 per row, already checked by the caller (finite, |p| <= 1); null drops them.
int node_set_priors(Node* h, const float* priors, int64_t n, const char** why);
// ROW UPDATES: rows[0..count) (checked by the caller: inside the catalogue, no duplicates) take feats[i * 12 ..].  The backend
// derives nothing from a row ahead of a query, so the host matrix is all there is to rewrite; results already computed
// (tickets of the stream) stay what they were.
int node_update_rows(Node* h, const int64_t* rows, int64_t count, const float* feats, const char** why);
int node_set_window(Node* h, int window, const char** why);
int node_enqueue(Node* h, const float* q12, int64_t exclude, int topn, int64_t* ticket, const char** why);
int node_flush(Node* h);
int node_wait(Node* h, int64_t ticket, int64_t* out_idx, float* out_score, int* out_count, const char** why);
void node_stream_stats(const Node* h, int64_t* queries, int64_t* windows, int64_t* host_ns);

}  // namespace mi355cpu
