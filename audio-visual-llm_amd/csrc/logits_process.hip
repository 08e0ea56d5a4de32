// Logits processors of HF's generate() between the token step and the selection kernel (argmax_rows / sample_rows / beam_topk), in place on
// [rows, V] scores: RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor (transformers
// generation/logits_process.py), in the order GenerationMixin._get_logits_processor builds them.  With inputs_embeds and no input_ids HF's
// processors see the generated tokens only, so the history of a row is its n generated tokens (pad tokens of a finished row included).
//
// One 1024-thread workgroup per row, thread i owns history position i (n <= MAX_HIST = 1024); the work is O(n) entries of the row:
//   0. optional (beam search): the row becomes its own log-softmax first, (x - max) - log(sum exp(x - max)) in fp32, because HF's beam search
//      applies the processors to log-probabilities: the normaliser is that of the unprocessed logits.  Three passes over V, reductions in
//      a fixed order (per-thread strided partials, wave butterflies, the waves' partials in wave order): the bits repeat from run to run.
//   1. penalty p != 1: thread i GATHERS v = s[hist[i]]; barrier; it SCATTERS v < 0 ? v * p : v / p (IEEE division).  A token that occurs
//      several times is written several times with the same value computed from the unprocessed score: penalised once, as HF's
//      gather / where / scatter does.  Barrier.
//   2. n-gram size g > 0 and n + 1 >= g: thread i <= n - g compares hist[i : i+g-1] with the last g-1 tokens and on a match stores -inf at
//      hist[i+g-1] (g == 1: every token of the history).
//   3. n < min_new and the model has an EOS id: -inf at eos.
// Steps 2 and 3 store the same value, so their order among threads is irrelevant; integer compares only.  History entries outside [0, V)
// are never used as an index and match nothing.
// `append` (optional, int64 [rows]): the token the selection kernel produced for position n-1, which this launch stores into the history
// before using it: the token loop keeps its history on the device without a copy launch of its own.
#include "common.h"
#include "avllm_internal.h"

namespace {

constexpr int NT = 1024, MAX_HIST = 1024;

template <typename T>
__global__ __launch_bounds__(NT) void process_kernel(T* scores, long ld, int V, int64_t* history, long ldh,
                                                     const int64_t* __restrict__ append, int cur, const int* __restrict__ cur_dev, float penalty,
                                                     int ngram, int min_new, long long eos, int log_softmax) {
    __shared__ int tok[MAX_HIST];                  // history as vocabulary indices, -1 = outside [0, V)
    __shared__ float red[NT / AV_WAVE];
    const int row = blockIdx.x, tid = threadIdx.x;
    T* s = scores + (long)row * ld;
    int n = cur + (cur_dev ? *cur_dev : 0);
    const int cap = ldh < MAX_HIST ? (int)ldh : MAX_HIST;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    if (tid < n) {
        int64_t* h = history + (long)row * ldh;
        long long t;
        if (append && tid == n - 1) { t = append[row]; h[tid] = t; }
        else t = h[tid];
        tok[tid] = (t >= 0 && t < V) ? (int)t : -1;
    }
    if (log_softmax) {
        float m = -INFINITY;
        for (int i = tid; i < V; i += NT) m = fmaxf(m, to_f(s[i]));
        m = block_max(m, red);
        float z = 0.f;
        for (int i = tid; i < V; i += NT) z += expf(to_f(s[i]) - m);
        z = block_sum(z, red);
        const float lz = logf(z);
        for (int i = tid; i < V; i += NT) s[i] = from_f<T>((to_f(s[i]) - m) - lz);
    }
    __syncthreads();                               // tok[] complete; the normalised row visible to every thread of the workgroup
    if (penalty != 1.0f) {
        const int t = tid < n ? tok[tid] : -1;
        const float v = t >= 0 ? to_f(s[t]) : 0.f;
        __syncthreads();                           // every gather before any scatter
        if (t >= 0) s[t] = from_f<T>(v < 0.f ? v * penalty : v / penalty);
        __syncthreads();                           // the bans below overwrite penalised scores, never the reverse
    }
    if (ngram > 0 && ngram <= n - tid) {
        const int last = n - ngram + 1;            // the last ngram-1 tokens start here
        bool match = true;
        for (int j = 0; j + 1 < ngram && match; ++j) match = tok[tid + j] == tok[last + j] && tok[tid + j] >= 0;
        const int t = tok[tid + ngram - 1];
        if (match && t >= 0) s[t] = from_f<T>(-INFINITY);
    }
    if (tid == 0 && n < min_new && eos >= 0 && eos < V) s[eos] = from_f<T>(-INFINITY);
}

}  // namespace

int av_logits_process(void* scores, long ld, long rows, int V, int64_t* history, long ldh, const int64_t* append, int cur, const int* cur_dev,
                      float penalty, int ngram, int min_new, long long eos, int log_softmax, int dtype, hipStream_t st) {
    AV_CHECK_ARG(scores && rows > 0 && V > 0 && ld >= V, "logits_process: bad args");
    AV_CHECK_ARG(dtype == AV_F32 || dtype == AV_BF16, "logits_process: dtype");
    AV_CHECK_ARG(!log_softmax || dtype == AV_F32, "logits_process: the log-softmax mode takes f32 rows");
    AV_CHECK_ARG(penalty > 0.f && penalty < INFINITY, "logits_process: repetition_penalty must be > 0 (got %g)", (double)penalty);
    AV_CHECK_ARG(ngram >= 0, "logits_process: no_repeat_ngram_size must be >= 0 (got %d)", ngram);
    AV_CHECK_ARG(min_new >= 0, "logits_process: min_new_tokens must be >= 0 (got %d)", min_new);
    AV_CHECK_ARG(cur >= 0 && ldh >= 0, "logits_process: history length %d, row stride %ld", cur, ldh);
    AV_CHECK_ARG(cur <= MAX_HIST, "logits_process: a history of %d tokens (at most %d are supported)", cur, MAX_HIST);
    AV_CHECK_ARG(cur <= ldh, "logits_process: history length %d > row stride %ld", cur, ldh);
    // the length in device memory cannot be checked here: the kernel clamps it to the row stride, which must then be within the limit
    AV_CHECK_ARG(!cur_dev || ldh <= MAX_HIST, "logits_process: a history of up to %ld tokens (at most %d are supported)", ldh, MAX_HIST);
    AV_CHECK_ARG(history || (cur == 0 && !cur_dev), "logits_process: null history");
    AV_CHECK_ARG(rows < (1L << 31), "logits_process: rows");
    if (penalty == 1.0f && ngram == 0 && min_new == 0 && !log_softmax && !append) return AV_OK;
    if (dtype == AV_F32)
        hipLaunchKernelGGL(process_kernel<float>, dim3((unsigned)rows), dim3(NT), 0, st, (float*)scores, ld, V, history, ldh, append, cur, cur_dev,
                           penalty, ngram, min_new, eos, log_softmax);
    else
        hipLaunchKernelGGL(process_kernel<bf16>, dim3((unsigned)rows), dim3(NT), 0, st, (bf16*)scores, ld, V, history, ldh, append, cur, cur_dev,
                           penalty, ngram, min_new, eos, log_softmax);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
