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
//
// With device tables in the descriptor (process_kernel<T, true>, the same launch) it adds SequenceBiasLogitsProcessor,
// NoBadWordsLogitsProcessor, SuppressTokensLogitsProcessor and SuppressTokensAtBeginLogitsProcessor at their places in HF's order:
//   0. log-softmax   0b. sequence bias   1. penalty   2. n-gram ban   2b. bad words   3. min_new_tokens   4. suppress   5. begin-suppress
//   0b. sequence bias: entries (tokens[L], fp32 bias), L <= MAX_SEQ_LEN, SORTED by the caller so that the entries with one last token are
//      adjacent: the length-1 entry first, the longer ones in the order of HF's dict.  An entry applies when L == 1, or when L <= n (HF's
//      test, not L-1 <= n) and the row's last L-1 tokens equal its first L-1.  The thread that owns the first entry of a group walks the
//      group, sums the biases of the entries that apply in fp32 in that order starting from +0 (HF's `bias` tensor) and stores
//      s[last] + total once: no atomics, the same bits every run, bf16 rounded once.  A barrier follows: the penalty reads biased scores.
//   2b. bad words: the same test per entry, one thread each; a match stores -inf at the entry's last token (s + -inf).
//   4. -inf at every id of the suppress list (any length up to V, ids unique).   5. the same for the begin list when n == 0: with
//      inputs_embeds HF's begin_index is the prompt length 0.
// Stages 2 to 5 only store -inf and sit behind the barriers of stages 0b and 1, so their order among threads is irrelevant.  Table ids
// outside [0, V) are never used as an index.  The history, and with it the MAX_HIST limit, is needed only by stages 1 to 3, by append and
// by entries longer than one token; without those the launch takes n from cur / cur_dev alone and a null history.
#include "common.h"
#include "avllm_internal.h"

namespace {

constexpr int NT = 1024, MAX_HIST = 1024, MAX_SEQS = AVLLM_LOGITS_MAX_SEQUENCES, MAX_SEQ_LEN = AVLLM_LOGITS_MAX_SEQUENCE_LEN;

struct SeqTable { const int* tok; const int* len; const float* bias; int n; };      // tok [n, MAX_SEQ_LEN], entry i's ids in its first len[i]
struct Tables { SeqTable bias, bad; const int* suppress; int n_suppress; const int* begin; int n_begin; };

// Last token of entry i, or -1 when the entry's length is outside [1, MAX_SEQ_LEN].
__device__ inline int seq_last(const SeqTable& t, int i) {
    const int L = t.len[i];
    return (L >= 1 && L <= MAX_SEQ_LEN) ? t.tok[(long)i * MAX_SEQ_LEN + L - 1] : -1;
}

// HF's SequenceBiasLogitsProcessor test for entry i on a row of n generated tokens (tok[0..n), -1 = outside the vocabulary).
__device__ inline bool seq_applies(const SeqTable& t, int i, const int* tok, int n) {
    const int L = t.len[i];
    if (L == 1) return true;
    if (L < 1 || L > MAX_SEQ_LEN || L > n) return false;
    const int* e = t.tok + (long)i * MAX_SEQ_LEN;
    const int* h = tok + n - (L - 1);
    for (int j = 0; j + 1 < L; ++j)
        if (h[j] != e[j] || e[j] < 0) return false;
    return true;
}

// -inf at every id of a list (ids outside [0, V) skipped).  Eight independent id loads are in flight before their stores: a full-vocabulary
// list is V stores from one workgroup, and one load-store pair at a time leaves that bound by latency.
template <typename T>
__device__ inline void ban_ids(T* s, const int* __restrict__ ids, int n, int V, int tid) {
    constexpr int U = 8;
    int i = tid;
    for (; i + (U - 1) * NT < n; i += U * NT) {
        int t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = ids[i + u * NT];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (t[u] >= 0 && t[u] < V) s[t[u]] = from_f<T>(-INFINITY);
    }
    for (; i < n; i += NT) {
        const int t = ids[i];
        if (t >= 0 && t < V) s[t] = from_f<T>(-INFINITY);
    }
}

template <typename T, bool EX>
__global__ __launch_bounds__(NT) void process_kernel(T* scores, long ld, int V, int64_t* history, long ldh,
                                                     const int64_t* __restrict__ append, int cur, const int* __restrict__ cur_dev, float penalty,
                                                     int ngram, int min_new, long long eos, int log_softmax, Tables tb) {
    __shared__ int tok[MAX_HIST];                  // history as vocabulary indices, -1 = outside [0, V)
    __shared__ float red[NT / AV_WAVE];
    const int row = blockIdx.x, tid = threadIdx.x;
    T* s = scores + (long)row * ld;
    int n = cur + (cur_dev ? *cur_dev : 0);
    const bool begin = n <= 0;
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
    if (EX && tb.bias.n > 0) {
        for (int i = tid; i < tb.bias.n; i += NT) {
            const int t = seq_last(tb.bias, i);
            if (t < 0 || t >= V || (i > 0 && seq_last(tb.bias, i - 1) == t)) continue;      // only the first entry of a group works
            float total = 0.f;
            for (int j = i; j < tb.bias.n && seq_last(tb.bias, j) == t; ++j)
                if (seq_applies(tb.bias, j, tok, n)) total += tb.bias.bias[j];
            s[t] = from_f<T>(to_f(s[t]) + total);
        }
        __syncthreads();                           // the penalty and the bans below see biased scores
    }
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
    if (EX) {
        for (int i = tid; i < tb.bad.n; i += NT) {
            const int t = seq_last(tb.bad, i);
            if (t >= 0 && t < V && seq_applies(tb.bad, i, tok, n)) s[t] = from_f<T>(-INFINITY);
        }
    }
    if (tid == 0 && n < min_new && eos >= 0 && eos < V) s[eos] = from_f<T>(-INFINITY);
    if (EX) {
        ban_ids(s, tb.suppress, tb.n_suppress, V, tid);
        if (begin) ban_ids(s, tb.begin, tb.n_begin, V, tid);
    }
}

template <bool EX>
void launch(void* scores, long ld, long rows, int V, int64_t* history, long ldh, const int64_t* append, int cur, const int* cur_dev, float penalty,
            int ngram, int min_new, long long eos, int log_softmax, int dtype, const Tables& tb, hipStream_t st) {
    if (dtype == AV_F32)
        hipLaunchKernelGGL((process_kernel<float, EX>), dim3((unsigned)rows), dim3(NT), 0, st, (float*)scores, ld, V, history, ldh, append, cur,
                           cur_dev, penalty, ngram, min_new, eos, log_softmax, tb);
    else
        hipLaunchKernelGGL((process_kernel<bf16, EX>), dim3((unsigned)rows), dim3(NT), 0, st, (bf16*)scores, ld, V, history, ldh, append, cur,
                           cur_dev, penalty, ngram, min_new, eos, log_softmax, tb);
}

}  // namespace

// The one host entry: avllm_logits_process fills a descriptor with no tables and comes here too.  process_kernel<T, true> when any table is
// non-empty, process_kernel<T, false> otherwise; no launch when there is nothing to do.
int av_logits_process(const avllm_logits_proc_desc* d, hipStream_t st) {
    AV_CHECK_ARG(d, "logits_process: null descriptor");
    const float penalty = d->repetition_penalty;
    const int ngram = d->no_repeat_ngram_size, min_new = d->min_new_tokens, cur = d->cur, V = d->V;
    AV_CHECK_ARG(d->scores && d->rows > 0 && V > 0 && d->ld >= V, "logits_process: bad args");
    AV_CHECK_ARG(d->dtype == AV_F32 || d->dtype == AV_BF16, "logits_process: dtype");
    AV_CHECK_ARG(!d->log_softmax || d->dtype == AV_F32, "logits_process: the log-softmax mode takes f32 rows");
    AV_CHECK_ARG(penalty > 0.f && penalty < INFINITY, "logits_process: repetition_penalty must be > 0 (got %g)", (double)penalty);
    AV_CHECK_ARG(ngram >= 0, "logits_process: no_repeat_ngram_size must be >= 0 (got %d)", ngram);
    AV_CHECK_ARG(min_new >= 0, "logits_process: min_new_tokens must be >= 0 (got %d)", min_new);
    AV_CHECK_ARG(cur >= 0 && d->ldh >= 0, "logits_process: history length %d, row stride %ld", cur, (long)d->ldh);
    AV_CHECK_ARG(d->rows < (1L << 31), "logits_process: rows");
    AV_CHECK_ARG(d->n_bias >= 0 && d->n_bias <= MAX_SEQS, "logits_process: sequence_bias has %d sequences (at most %d are supported)", d->n_bias, MAX_SEQS);
    AV_CHECK_ARG(d->n_bad >= 0 && d->n_bad <= MAX_SEQS, "logits_process: bad_words_ids has %d sequences (at most %d are supported)", d->n_bad, MAX_SEQS);
    AV_CHECK_ARG(!d->n_bias || (d->bias_tokens && d->bias_lengths && d->bias_values), "logits_process: null sequence_bias table");
    AV_CHECK_ARG(!d->n_bad || (d->bad_tokens && d->bad_lengths), "logits_process: null bad_words_ids table");
    AV_CHECK_ARG(!d->n_bias || (d->bias_max_len >= 1 && d->bias_max_len <= MAX_SEQ_LEN),
                 "logits_process: a sequence_bias sequence of %d tokens (1 to %d are supported)", d->bias_max_len, MAX_SEQ_LEN);
    AV_CHECK_ARG(!d->n_bad || (d->bad_max_len >= 1 && d->bad_max_len <= MAX_SEQ_LEN),
                 "logits_process: a bad_words_ids sequence of %d tokens (1 to %d are supported)", d->bad_max_len, MAX_SEQ_LEN);
    AV_CHECK_ARG(d->n_suppress >= 0 && d->n_suppress <= V && (!d->n_suppress || d->suppress),
                 "logits_process: suppress_tokens has %d ids (at most V = %d distinct ones)", d->n_suppress, V);
    AV_CHECK_ARG(d->n_begin_suppress >= 0 && d->n_begin_suppress <= V && (!d->n_begin_suppress || d->begin_suppress),
                 "logits_process: begin_suppress_tokens has %d ids (at most V = %d distinct ones)", d->n_begin_suppress, V);
    // the history is read by the three older processors, by append, and by table entries longer than one token
    const bool need_hist = penalty != 1.0f || ngram > 0 || min_new > 0 || d->append || (d->n_bias && d->bias_max_len > 1) ||
                           (d->n_bad && d->bad_max_len > 1);
    if (need_hist) {
        AV_CHECK_ARG(cur <= MAX_HIST, "logits_process: a history of %d tokens (at most %d are supported)", cur, MAX_HIST);
        AV_CHECK_ARG(cur <= d->ldh, "logits_process: history length %d > row stride %ld", cur, (long)d->ldh);
        // the length in device memory cannot be checked here: the kernel clamps it to the row stride, which must then be within the limit
        AV_CHECK_ARG(!d->cur_dev || d->ldh <= MAX_HIST, "logits_process: a history of up to %ld tokens (at most %d are supported)", (long)d->ldh,
                     MAX_HIST);
        AV_CHECK_ARG(d->history || (cur == 0 && !d->cur_dev), "logits_process: null history");
    }
    int64_t* const history = need_hist ? d->history : nullptr;
    const long ldh = history ? d->ldh : 0;
    const bool tables = d->n_bias || d->n_bad || d->n_suppress || d->n_begin_suppress;
    if (!tables && !need_hist && !d->log_softmax) return AV_OK;      // every processor off: nothing to do
    const Tables tb{SeqTable{d->bias_tokens, d->bias_lengths, d->bias_values, d->n_bias}, SeqTable{d->bad_tokens, d->bad_lengths, nullptr, d->n_bad},
                    d->suppress, d->n_suppress, d->begin_suppress, d->n_begin_suppress};
    (tables ? launch<true> : launch<false>)(d->scores, d->ld, d->rows, V, history, ldh, d->append, cur, d->cur_dev, penalty, ngram, min_new, d->eos,
                                            d->log_softmax, d->dtype, tb, st);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
