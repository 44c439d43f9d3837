// Host-side engine of the dual-AR LM (see lm_engine.h).  All device work goes through the hand-written kernels
// of lm_kernels.hip on ONE HIP stream; the per-frame inner loop (24 slow blocks + head + sample + 8 x (4 fast blocks
// + head + sample)) is captured once into a hipGraph and replayed with zero host round trips per frame.
//
// Reference call graph implemented here:
//   generate_blocking               fish_speech_core/lib/lm/generate/single_batch.rs:217-324
//   SingleBatchGenerator::{new,next} fish_speech_core/lib/lm/generate/single_batch.rs:31-214
//   DualARTransformer::forward_generate[_fast] / cache lifecycle   fish_speech_core/lib/lm/dual_ar.rs:574-700
#include "lm_engine.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <initializer_list>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include "fs_common.h"
#include "fs_kv_pages.h"
#include "fs_prefill_plan.h"
#include "fs_synth.h"
#include "lm_kernels.h"
#include "lm_persist.h"
#include "lm_persist_rows.h"
#include "safetensors.h"

namespace fs {

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    void alloc(size_t bytes) {
        free();
        n = bytes;
        if (bytes) FS_HIP(hipMalloc(&p, bytes));
    }
    void free() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { free(); }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// the repetition-penalty state (lm_kernels.h: RepPenState) of `rows` sampler rows, row after row: per codebook the mask and seen tables
// over the codebook, the 17-word ring and its 2 meta words
struct RepPenBufs {
    DevBuf mask, seen, ring, meta;
    size_t per_row[4] = {0, 0, 0, 0};  // elements of one row in each of the four
    void alloc(size_t rows, size_t n_codebooks, size_t codebook_size) {
        per_row[0] = per_row[1] = n_codebooks * codebook_size; per_row[2] = n_codebooks * 17; per_row[3] = n_codebooks * 2;
        mask.alloc(sizeof(float) * rows * per_row[0]); seen.alloc(rows * per_row[1]);
        ring.alloc(sizeof(int) * rows * per_row[2]); meta.alloc(sizeof(int) * rows * per_row[3]);
    }
    RepPenState view(size_t row) const {
        return RepPenState{mask.as<float>() + row * per_row[0], seen.as<uint8_t>() + row * per_row[1], ring.as<int>() + row * per_row[2],
                           meta.as<int>() + row * per_row[3]};
    }
};

// One collector kind of a session (fs_slot_book.h; E = HidSlot: fs_lm_session_add_hidden, ScoreSlot: fs_lm_session_add_scored): the host
// mirror of the per-slot table + the handle's buffer pool, the device table the step's node reads (allocated once per handle: the
// captured step graphs hold its address), and the landing place of the end-of-chunk copy of the counts
void* slot_buf_alloc(size_t n) { void* p = nullptr; return hipMalloc(&p, n) == hipSuccess ? p : nullptr; }
void slot_buf_free(void* p) { (void)hipFree(p); }
template <typename E>
struct SlotTab {
    SlotBook<E> book{&slot_buf_alloc, &slot_buf_free};
    DevBuf dev;
    std::vector<E> stage;
};

struct TensorDesc {
    std::string name;      // reference tensor name (dual_ar.rs loader)
    int64_t rows, cols;
    bool is_vec;           // f32 norm vector (device f32) vs WT matrix
    bool is_emb;           // embedding table: stored in KVT<WT> (bf16 when the matrices are fp8)
    size_t offset;         // byte offset in the arena (destination base of the possibly interleaved slab)
    size_t scale_off;      // fp8 matrices: byte offset of the per-row f32 scale slab (same row mapping)
    int row_mul, row_off;  // destination row = r * row_mul + row_off
    float mean;
    double stdv;
};


// The persistent kernels need all of their 256 workgroups co-resident; two such launches on one GPU -- from two handles of one process
// OR from two processes -- could each hold half of the CUs and wait for the other half forever (until their spin limits).  One call at a
// time may use them per PHYSICAL device: an in-process mutex (threads) plus an advisory flock() on a per-device file keyed by the PCI bus
// id (processes; the kernel drops the lock when its holder dies).  A call that does not get the lock takes the per-node graphs instead;
// FISHRT_PERSIST_WAIT=1 makes it wait for the holder (two ranks sharing one GPU in a rehearsal: both deterministic, one after the other).
class PersistLock {
  public:
    void bind(int device) {
        std::call_once(once_, [&] {
            char bus[64] = {0};
            if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) snprintf(bus, sizeof(bus), "dev%d", device);
            for (char* c = bus; *c; ++c) if (*c == ':' || *c == '/') *c = '_';
            // The file must be visible to EVERY process that can reach the GPU (another user's process holding half the CUs is exactly the
            // case the lock exists for), so it lives in a shared directory.  ADVICE r5: never follow a planted symlink (O_NOFOLLOW), accept
            // only a regular file, and leave its mode alone unless this process created it (fchmod fails for a non-owner anyway).
            for (const char* dir : {"/dev/shm", "/tmp"}) {
                const std::string path = std::string(dir) + "/fishrt-persist-" + bus + ".lock";
                int fd = open(path.c_str(), O_RDWR | O_CLOEXEC | O_NOFOLLOW);
                if (fd < 0 && errno == ENOENT) {
                    fd = open(path.c_str(), O_CREAT | O_EXCL | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0666);
                    if (fd >= 0) (void)fchmod(fd, 0666);
                    else if (errno == EEXIST) fd = open(path.c_str(), O_RDWR | O_CLOEXEC | O_NOFOLLOW);  // (lost the creation race)
                }
                if (fd < 0) continue;
                struct stat st;
                if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); continue; }
                fd_ = fd;
                break;
            }  // (no usable file: the lock stays process-local)
        });
    }
    bool try_lock() {
        {
            std::lock_guard<std::mutex> g(mm_);
            if (held_) return false;
            held_ = true;
        }
        if (fd_ >= 0 && flock(fd_, LOCK_EX | LOCK_NB) != 0) { release_local(); return false; }
        return true;
    }
    // FISHRT_PERSIST_WAIT: wait for the holder -- but not forever (anybody can hold an advisory lock on a shared file): the wait
    // is bounded (the variable's value in seconds; 1 = the default of 600), after which the caller runs on the per-node graphs like a
    // caller that never waited.  Returns whether the lock was taken.
    bool lock_for(double seconds) {
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(seconds);
        {
            std::unique_lock<std::mutex> g(mm_);
            if (!cv_.wait_until(g, deadline, [&] { return !held_; })) return false;
            held_ = true;
        }
        if (fd_ < 0) return true;
        for (;;) {
            if (flock(fd_, LOCK_EX | LOCK_NB) == 0) return true;
            if (std::chrono::steady_clock::now() >= deadline) { release_local(); return false; }
            usleep(500);
        }
    }
    // (no lock(): std::unique_lock is only ever built with try_to_lock, adopt_lock or defer_lock on this -- acquire_persist -- and a wait
    // that can time out has no business behind an interface that promises the lock)
    // (a binary semaphore, not a std::mutex: a row session takes it in session_begin and gives it back in session_end, possibly on another thread)
    void unlock() {
        if (fd_ >= 0) (void)flock(fd_, LOCK_UN);
        release_local();
    }

  private:
    void release_local() {
        { std::lock_guard<std::mutex> g(mm_); held_ = false; }
        cv_.notify_one();
    }
    std::mutex mm_;
    std::condition_variable cv_;
    bool held_ = false;
    std::once_flag once_;
    int fd_ = -1;
};
PersistLock& persist_mutex(int device) {
    static PersistLock m[64];
    m[device & 63].bind(device);
    return m[device & 63];
}
// try (default) or wait (FISHRT_PERSIST_WAIT = seconds; 1 = 600 s) for the device's persistent kernels
std::unique_lock<PersistLock> acquire_persist(int device) {
    PersistLock& pl = persist_mutex(device);
    if (const char* w = getenv("FISHRT_PERSIST_WAIT")) {
        const double secs = atof(w) > 1.0 ? atof(w) : 600.0;
        if (pl.lock_for(secs)) return std::unique_lock<PersistLock>(pl, std::adopt_lock);
        return std::unique_lock<PersistLock>(pl, std::defer_lock);
    }
    return std::unique_lock<PersistLock>(pl, std::try_to_lock);
}

constexpr int kRows = 256;     // static-batch generator: max sequences per step (32-row MFMA panels; <= kPartRows)
constexpr int kRowsCap = 2048; // row capacity of the MFMA row buffers: prompt tokens per prefill pass (one sequence, or a group of
                               // left-padded static-batch prompts)
constexpr int kPartRows = 512; // rows of the chunked-attention partials buffer (static-batch steps; prefill passes when head_dim != 64)

// One set of the MFMA row path's activation buffers (kRowsCap rows), with the stream its passes run on and the prompt staged for them.
// A handle has two: the main lane on the engine stream -- its buffers are also the static-batch decode steps', whose captured graphs
// hold their addresses, so a lane allocates once and never again -- and the join lane on a session's prefill stream.
struct PrefillLane {
    hipStream_t& st;
    DevBuf x, q, slab, a, a2, ss, c, part;  // RowsCtx: X, Q, P, A, A2, ss, C, part
    DevBuf prompt;                          // the staged prompt [C + 1][cols] (the join lane's group passes: [S][C + 1][Lp])
    RowsCtx base = {};                      // what no pass changes of a RowsCtx
    explicit PrefillLane(hipStream_t& s) : st(s) {}
    void ensure(const fs_model_args& m, int down_split, int n_chunks, const float* cos_t, const float* sin_t) {
        if (x.p) return;
        x.alloc(sizeof(float) * kRowsCap * m.dim);
        q.alloc(sizeof(float) * kRowsCap * m.dim);
        slab.alloc(sizeof(float) * down_split * kRowsCap * m.dim);
        a.alloc(sizeof(uint16_t) * 2 * kRowsCap * m.dim);
        a2.alloc(sizeof(uint16_t) * 2 * kRowsCap * m.dim);
        ss.alloc(sizeof(float) * kRowsCap * (m.dim / 16));
        c.alloc(sizeof(uint16_t) * 2 * kRowsCap * m.intermediate_size);
        part.alloc(sizeof(float) * kPartRows * (size_t)m.n_head * n_chunks * (m.head_dim + 2));
        for (DevBuf* bf : {&x, &a, &a2, &ss, &c, &part}) FS_HIP(hipMemsetAsync(bf->p, 0, bf->n, st));
        base.X = x.as<float>(); base.Q = q.as<float>(); base.part = part.as<float>(); base.P = slab.as<float>();
        base.Mcap = kRowsCap; base.part_rows = kPartRows; base.down_split = down_split;
        base.A = a.as<uint16_t>(); base.C = c.as<uint16_t>();
        base.A2 = a2.as<uint16_t>(); base.ss = ss.as<float>();
        base.cos_t = cos_t; base.sin_t = sin_t;
        base.n_chunks_max = n_chunks; base.nc_launch = n_chunks;
    }
    RowsCtx ctx(const SeqState* state, int pos_step, int pt_stride) const {
        RowsCtx r = base;
        r.state = state; r.pos_step = pos_step; r.pt_stride = pt_stride;
        return r;
    }
    // the prompt of the lane's next pass, on its stream (the source must outlive the copy; a pass that still reads the buffer has been waited for)
    void stage_prompt(const uint32_t* src, size_t n) {
        if (prompt.n < sizeof(uint32_t) * n) prompt.alloc(sizeof(uint32_t) * n);
        FS_HIP(hipMemcpyAsync(prompt.p, src, sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
    }
};

}  // namespace

template <typename WT>
class LM final : public LMBase {
    using KT = KVT<WT>;  // KV cache / embedding storage type
    static constexpr bool kFp8 = std::is_same<WT, fp8_t>::value;

  public:
    LM(const fs_model_args& a, const fs_token_cfg& t, int device, int max_batch) : a_(a), t_(t), device_(device), B_(max_batch) {
        FS_REQUIRE(max_batch >= 1, "max_batch must be >= 1");
        FS_REQUIRE(a.dim == a.n_head * a.head_dim, "dim must equal n_head * head_dim (dual_ar.rs:173,381)");
        FS_REQUIRE(a.n_head % a.n_local_heads == 0, "n_head must be a multiple of n_local_heads");
        FS_REQUIRE(a.head_dim % 8 == 0 && a.num_codebooks + 1 <= 16, "unsupported head_dim / num_codebooks");
        FS_REQUIRE(t.im_end_id < (uint32_t)a.vocab_size, "im_end_id outside the vocabulary");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            throw Error("no HIP device visible: libfishrt has no CPU fallback (MI355X / gfx950 required)");
        FS_REQUIRE(device >= 0 && device < ndev, "device_id out of range");
        FS_HIP(hipSetDevice(device));
        hipDeviceProp_t prop;
        FS_HIP(hipGetDeviceProperties(&prop, device));
        if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
            throw Error(std::string("libfishrt kernels are built for gfx950 only; device reports ") + prop.gcnArchName);
        FS_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
        d_.dim = a.dim; d_.inter = a.intermediate_size; d_.H = a.n_head; d_.Hk = a.n_local_heads; d_.Dh = a.head_dim;
        d_.n_rep = a.n_head / a.n_local_heads; d_.eps = a.norm_eps;
        legacy_ = !t.has_semantic_end;  // Fish <= 1.4: slow token is a 2-way {pad, im_end} draw (single_batch.rs:104-124)
        // generic DualAR token layout (utils.rs:17-30): <|im_end|> does not directly precede the semantic range -- the slow head's
        // candidates are [im_end] ++ [semantic_start, V) (literally: any control token behind the range, <|im_end|> itself included, stays a
        // candidate), gathered into one head image at load time
        generic_ = !legacy_ && t.im_end_id + 1 != t.semantic_start_id;
        if (!legacy_) FS_REQUIRE(t.semantic_start_id >= 1 && t.semantic_start_id < (uint32_t)a.vocab_size, "semantic_start_id outside the vocabulary");
        n_audio_ = legacy_ ? 2 : (generic_ ? a.vocab_size - (int)t.semantic_start_id + 1 : a.vocab_size - (int)t.im_end_id);
        if (legacy_) FS_REQUIRE(t.pad_id < (uint32_t)a.vocab_size, "pad_id outside the vocabulary");
        plan_tensors();
        alloc_runtime();
        for (auto& e : ev_) FS_HIP(hipEventCreate(&e));
        for (auto& e : ev_batch_) FS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    ~LM() override {
        (void)hipSetDevice(device_);
        (void)hipStreamSynchronize(st_);
        destroy_graphs();
        for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
        for (auto& e : ev_batch_) if (e) (void)hipEventDestroy(e);
        if (h_pin_) (void)hipHostFree(h_pin_);
        if (ev_pf_) (void)hipEventDestroy(ev_pf_);
        for (hipEvent_t e : ev_pft_) if (e) (void)hipEventDestroy(e);
        if (st_pf_) (void)hipStreamDestroy(st_pf_);
        if (st_) (void)hipStreamDestroy(st_);
    }

    // ------------------------------------------------------------------------------------------ weights
    void load_synthetic(uint64_t seed) override {
        use_device();
        // a bf16 (or fp8) checkpoint holds bf16-rounded vectors / embeddings; fp8 matrices are quantised from the raw values
        const int round_bf16 = std::is_same<WT, float>::value ? 0 : 1;
        uint8_t* base = arena_.as<uint8_t>();
        for (const auto& td : tensors_) {
            const uint64_t key = synth_fnv1a64(td.name.c_str()) ^ seed;
            const float sc = synth_scale(td.stdv);
            if (td.is_vec)
                launch_synth_fill<float>((float*)(base + td.offset), key, td.rows, td.cols, 1, 0, td.mean, sc, round_bf16, st_);
            else if (td.is_emb)
                launch_synth_fill<KT>((KT*)(base + td.offset), key, td.rows, td.cols, td.row_mul, td.row_off, td.mean, sc, round_bf16, st_);
            else if constexpr (kFp8)
                launch_synth_quant_fp8(base + td.offset, (float*)(base + td.scale_off), key, td.rows, td.cols, td.row_mul, td.row_off,
                                       td.mean, sc, st_);
            else
                launch_synth_fill<WT>((WT*)(base + td.offset), key, td.rows, td.cols, td.row_mul, td.row_off, td.mean, sc, round_bf16, st_);
        }
        FS_HIP(hipStreamSynchronize(st_));
        loaded_ = true;
        fp_valid_ = false;
        refresh_legacy_head();
        pack_persist();
    }

    void load_safetensors(const std::string& path) override {
        use_device();
        SafeTensors st(path);
        DevBuf stage;
        std::vector<float> host;
        for (const auto& td : tensors_) {
            std::string name = td.name;
            if (name == "output.weight" && a_.tie_word_embeddings) name = "embeddings.weight";  // dual_ar.rs:482-486
            // exact shape, as candle's VarBuilder::get: [rows, cols] for matrices / embeddings, [n] for norm vectors (a transposed tensor
            // of the same element count is an error, not a silent load)
            const StTensor* t = &st.get(name, td.is_vec ? std::vector<int64_t>{td.cols} : std::vector<int64_t>{td.rows, td.cols});
            host.resize((size_t)t->numel());
            SafeTensors::to_f32(*t, host.data());
            if (stage.n < host.size() * 4) stage.alloc(host.size() * 4);
            FS_HIP(hipMemcpyAsync(stage.p, host.data(), host.size() * 4, hipMemcpyHostToDevice, st_));
            uint8_t* base = arena_.as<uint8_t>();
            if (td.is_vec)
                launch_convert_rows<float>((float*)(base + td.offset), stage.as<float>(), td.rows, td.cols, 1, 0, st_);
            else if (td.is_emb)
                launch_convert_rows<KT>((KT*)(base + td.offset), stage.as<float>(), td.rows, td.cols, td.row_mul, td.row_off, st_);
            else if constexpr (kFp8)
                launch_quant_rows_fp8(base + td.offset, (float*)(base + td.scale_off), stage.as<float>(), td.rows, td.cols, td.row_mul,
                                      td.row_off, st_);
            else
                launch_convert_rows<WT>((WT*)(base + td.offset), stage.as<float>(), td.rows, td.cols, td.row_mul, td.row_off, st_);
            FS_HIP(hipStreamSynchronize(st_));
        }
        loaded_ = true;
        fp_valid_ = false;
        refresh_legacy_head();
        pack_persist();
    }

    // The arena is a pure function of (model args, token config, dtype, checkpoint): one rank loads the checkpoint, the others receive
    // the bytes (ncclBroadcast over xGMI instead of N disk reads + N conversions) and derive the load-time extras themselves.
    void weights_arena(void** dev_ptr, size_t* bytes) override {
        use_device();
        FS_HIP(hipStreamSynchronize(st_));
        *dev_ptr = arena_.p; *bytes = arena_bytes_;
    }
    void weights_adopt() override {
        use_device();
        FS_REQUIRE(!sess_active_, "the handle is in session mode (fs_lm_session_end first)");
        FS_HIP(hipDeviceSynchronize());  // the bytes were written by another stream (the communicator's)
        loaded_ = true;
        fp_valid_ = false;
        refresh_legacy_head();
        pack_persist();
    }

    // ------------------------------------------------------------------------------------------ teacher-forced API
    void forward_generate(const uint32_t* toks, int B, int L, int input_pos, float* logits, float* hidden) override {
        use_device();
        require_loaded();
        FS_REQUIRE(!sess_active_, "the handle is in session mode (fs_lm_session_end first)");
        FS_REQUIRE(B >= 1 && B <= B_, "batch size exceeds the handle's max_batch");
        FS_REQUIRE(L >= 1, "empty input");
        const int C1 = a_.num_codebooks + 1;
        for (int b = 1; b < B; ++b) FS_REQUIRE(seq_len_[b] == seq_len_[0], "KV cache length differs across batch rows");
        if (input_pos + L > a_.max_seq_len) throw Error("input_pos + seq_len exceeds max_seq_len (dual_ar.rs:623-624)");
        validate_tokens(toks, (size_t)B * C1 * L, B, L);
        std::vector<float> lg, hd;
        for (int b = 0; b < B; ++b) {
            ensure_capacity(b, seq_len_[b] + L);
            FS_HIP(hipMemcpyAsync(main_.prompt.p, toks + (size_t)b * C1 * L, sizeof(uint32_t) * C1 * L, hipMemcpyHostToDevice, st_));
            SeqState s = {};
            s.pos = seq_len_[b]; s.rope_off = input_pos - seq_len_[b]; s.prompt_L = L;
            FS_HIP(hipMemcpyAsync(state(b), &s, sizeof(s), hipMemcpyHostToDevice, st_));
            prefill_tokens(b, L, /*use_graph=*/false);
            seq_len_[b] += L;
            if (hidden) FS_HIP(hipMemcpyAsync(hidden + (size_t)b * a_.dim, x(b), sizeof(float) * a_.dim, hipMemcpyDeviceToHost, st_));
            if (logits) {
                LmKernels<WT>::head(d_, x(b), norm_w_, out_w_, out_s_, a_.vocab_size, d_logits_slow_.as<float>(), st_);
                FS_HIP(hipMemcpyAsync(logits + (size_t)b * a_.vocab_size, d_logits_slow_.p, sizeof(float) * a_.vocab_size,
                                      hipMemcpyDeviceToHost, st_));
            }
            FS_HIP(hipStreamSynchronize(st_));
        }
    }

    void forward_generate_fast(const float* xin, int B, int input_pos, float* logits) override {
        use_device();
        require_loaded();
        FS_REQUIRE(B >= 1 && B <= B_, "batch size exceeds the handle's max_batch");
        if (input_pos >= a_.max_seq_len) throw Error("input_pos exceeds max_seq_len");
        for (int b = 0; b < B; ++b) {
            FS_REQUIRE(fast_len_[b] < 8, "fast decoder KV holds at most 8 positions per frame (num_codebooks)");
            FS_HIP(hipMemcpyAsync(xf(b), xin + (size_t)b * a_.dim, sizeof(float) * a_.dim, hipMemcpyHostToDevice, st_));
            enqueue_fast_layers(b, fast_len_[b], input_pos);
            LmKernels<WT>::head(d_, xf(b), fast_norm_w_, fast_out_w_, fast_out_s_, a_.codebook_size, d_logits_fast_.as<float>(), st_);
            FS_HIP(hipMemcpyAsync(logits + (size_t)b * a_.codebook_size, d_logits_fast_.p, sizeof(float) * a_.codebook_size,
                                  hipMemcpyDeviceToHost, st_));
            FS_HIP(hipStreamSynchronize(st_));
            fast_len_[b] += 1;
        }
    }

    void fast_embed(const uint32_t* ids, int n, float* out) override {
        use_device();
        require_loaded();
        for (int i = 0; i < n; ++i) FS_REQUIRE(ids[i] < (uint32_t)a_.codebook_size, "fast embedding id out of range");
        DevBuf di, dout;
        di.alloc(sizeof(uint32_t) * n);
        dout.alloc(sizeof(float) * n * a_.dim);
        FS_HIP(hipMemcpyAsync(di.p, ids, sizeof(uint32_t) * n, hipMemcpyHostToDevice, st_));
        LmKernels<WT>::fast_embed(d_, fast_emb_, di.as<uint32_t>(), n, dout.as<float>(), st_);
        FS_HIP(hipMemcpyAsync(out, dout.p, sizeof(float) * n * a_.dim, hipMemcpyDeviceToHost, st_));
        FS_HIP(hipStreamSynchronize(st_));
    }

    void clear_fast() override { std::fill(fast_len_.begin(), fast_len_.end(), 0); }
    void clear_slow() override { for (int b = 0; b < B_; ++b) truncate(b, 0); }
    void clear_slow_until(int pos) override {
        FS_REQUIRE(pos >= 0, "negative position");
        for (int b = 0; b < B_; ++b) truncate(b, std::min(seq_len_[b], pos));
    }
    int kv_len() override { return seq_len_[0]; }
    // test hook (fs_lm_debug_capture / fs_lm_debug_read): the persistent fast decoder records, for the first n generator iterations of
    // each generate call, the (penalised, masked) logits every one of the 9 decisions of a frame saw and the index it picked
    void debug_capture(int n_frames) override {
        use_device();
        FS_REQUIRE(n_frames >= 0 && n_frames <= 4096, "bad frame count");
        FS_HIP(hipStreamSynchronize(st_));
        cap_frames_ = n_frames;
        if (n_frames) { d_cap_.alloc(sizeof(float) * (size_t)n_frames * 9 * 2048); FS_HIP(hipMemset(d_cap_.p, 0, d_cap_.n)); }
        else d_cap_ = DevBuf();
        destroy_graphs();  // the captured launches carry the buffer pointer (the row-path step graphs include the capture kernels only while the hook is armed)
        if (!n_frames) d_rcap_ = DevBuf();
    }
    void debug_read(float* out, int n_frames) override {
        use_device();
        FS_REQUIRE(n_frames >= 0 && n_frames <= cap_frames_, "more frames than were captured");
        FS_HIP(hipStreamSynchronize(st_));
        FS_HIP(hipMemcpy(out, d_cap_.p, sizeof(float) * (size_t)n_frames * 9 * 2048, hipMemcpyDeviceToHost));
    }
    // test hook (fs_lm_debug_read_kv): the cached K / V rows [t0, t0 + n) of slow layer `layer` of KV slot `slot`, as f32 [n][Hkv][Dh]
    void debug_read_kv(int slot, int layer, int t0, int n, float* k_out, float* v_out) override {
        use_device();
        FS_REQUIRE(slot >= 0 && slot < B_ && layer >= 0 && layer < a_.n_layer, "bad KV slot / layer");
        FS_REQUIRE(t0 >= 0 && n >= 0 && t0 + n <= (int)pages_.of(slot).size() * KV_PAGE, "rows outside the slot's KV pages");
        FS_HIP(hipStreamSynchronize(st_));
        const int Hk = a_.n_local_heads, Dh = a_.head_dim;
        std::vector<KT> pk(page_elems_), pv(page_elems_);
        const KT* kpool = kv_pool_.as<KT>() + (size_t)layer * 2 * n_pages_ * page_elems_;
        const KT* vpool = kpool + (size_t)n_pages_ * page_elems_;
        int have = -1;
        for (int t = t0; t < t0 + n; ++t) {
            const int pg = pages_.of(slot)[t >> 6];
            if (pg != have) {
                FS_HIP(hipMemcpy(pk.data(), kpool + (size_t)pg * page_elems_, sizeof(KT) * page_elems_, hipMemcpyDeviceToHost));
                FS_HIP(hipMemcpy(pv.data(), vpool + (size_t)pg * page_elems_, sizeof(KT) * page_elems_, hipMemcpyDeviceToHost));
                have = pg;
            }
            for (int g = 0; g < Hk; ++g)
                for (int d = 0; d < Dh; ++d) {
                    const size_t src = ((size_t)g * KV_PAGE + (t & 63)) * Dh + d, dst = ((size_t)(t - t0) * Hk + g) * Dh + d;
                    k_out[dst] = kv_f32(pk[src]); v_out[dst] = kv_f32(pv[src]);
                }
        }
    }
    static float kv_f32(float v) { return v; }
    static float kv_f32(bf16_t v) { return bf16_to_f32_host(v); }
    void debug_read_row(int row, float* out, int n_frames) override {
        use_device();
        FS_REQUIRE(row >= 0 && d_rcap_.p, "no row capture (fs_lm_debug_capture, then fs_lm_generate_multi / fs_lm_generate_batch / a session)");
        FS_REQUIRE(n_frames >= 0 && n_frames <= cap_frames_, "more frames than were captured");
        FS_REQUIRE(sizeof(float) * ((size_t)row + 1) * cap_frames_ * 9 * 2048 <= d_rcap_.n, "row beyond the captured rows");
        FS_HIP(hipStreamSynchronize(st_));
        FS_HIP(hipMemcpy(out, d_rcap_.as<float>() + (size_t)row * cap_frames_ * 9 * 2048, sizeof(float) * (size_t)n_frames * 9 * 2048, hipMemcpyDeviceToHost));
    }
    fs_gen_stats last_stats() override { return stats_; }
    void* stream() override { return (void*)st_; }

    // fs_lm_selftest("persist"): the persistent decode kernels of THIS binary against the per-node kernels, on the loaded
    // weights.  k_slow_persist requests weight slices through loads the compiler's wait-count pass does not see (lm_persist_slow.hip:
    // ps_load16_unseen) and k_fast_persist keeps 168 pinned weight registers per lane -- both depend on how hipcc allocates registers, so a
    // toolchain or flag change must be caught by running, not by reading.  Protocol: a 12-position prompt, 4 greedy frames on the
    // persistent path with the decision capture armed; then ONE teacher-forced per-node step (forward_generate at the position of frame 1,
    // fed frame 0's picks; forward_generate_fast on its hidden state) and a comparison of frame 1's captured logits -- the first slow
    // step k_slow_persist computed, the first codebook pass of k_fast_persist behind it -- with the per-node logits.  Both paths share the
    // prefill's K/V rows and differ in summation order only, so the bound is loose for rounding and tight for a wrong weight register:
    // 2e-2 x max(1, max |logit|).
    void selftest(const char* what) override {
        use_device();
        require_loaded();
        FS_REQUIRE(what && std::string(what) == "persist", "unknown handle self-test (known: \"persist\")");
        FS_REQUIRE(!sess_active_, "the handle is in session mode (fs_lm_session_end first)");
        FS_REQUIRE(cap_frames_ == 0, "decision capture is armed (fs_lm_debug_capture(lm, 0) first)");
        if (!persist_ok_ || !pslow_ok_) throw Error("self-test \"persist\": this handle has no persistent kernels (dtype / geometry / device)");
        const int C = a_.num_codebooks, C1 = C + 1, L = 12;
        const SampleCfg cfg = base_cfg();
        std::vector<uint32_t> prompt((size_t)C1 * L, 0u);
        const uint32_t n_text = std::max<uint32_t>(1u, std::min<uint32_t>(cfg.im_end_id, 1000u));
        for (int i = 0; i < L; ++i) prompt[i] = (uint32_t)((7919ull * (uint64_t)(i + 1) + 13ull) % n_text);
        clear_slow();
        debug_capture(2);
        struct Restore { LM* lm; ~Restore() { try { lm->debug_capture(0); lm->clear_slow(); lm->clear_fast(); } catch (...) {} } } restore{this};
        fs_sampling sa = {};
        sa.temp = 0.0; sa.top_p = 1.0; sa.top_k = 0; sa.repetition_penalty = 1.0f;
        std::vector<uint32_t> codes((size_t)C * 8, 0u);
        size_t nf = 0;
        generate(prompt.data(), L, L + 2, sa, 1, FS_GEN_IGNORE_EOS, codes.data(), 8, &nf, nullptr, nullptr, nullptr, 0, nullptr);
        if (stats_.kernels_per_frame != 2)
            throw Error("self-test \"persist\": the call did not take the persistent kernels (another handle of this GPU holds them?)");
        std::vector<float> cap((size_t)2 * 9 * 2048);
        debug_read(cap.data(), 2);
        std::vector<uint32_t> in(C1);
        in[0] = legacy_ ? cfg.pad_id : audio_tok(cfg, (int)cap[2047]);
        for (int c = 0; c < C; ++c) in[1 + c] = (uint32_t)cap[(size_t)(1 + c) * 2048 + 1024];
        clear_slow_until(L);
        std::vector<float> lg(a_.vocab_size), hid(a_.dim), lf(a_.codebook_size);
        forward_generate(in.data(), 1, 1, L, lg.data(), hid.data());
        clear_fast();
        forward_generate_fast(hid.data(), 1, 0, lf.data());
        const float* c_slow = cap.data() + (size_t)(9 + 0) * 2048;
        const float* c_fast = cap.data() + (size_t)(9 + 1) * 2048;
        float worst = 0.f, scale = 1.f;
        auto cmp = [&](float ref, float got) { scale = std::max(scale, std::fabs(ref)); worst = std::max(worst, std::fabs(ref - got)); };
        if (legacy_) { cmp(lg[cfg.pad_id], c_slow[0]); cmp(lg[cfg.im_end_id], c_slow[1]); }
        else for (int i = 1; i < n_audio_; ++i) cmp(lg[audio_tok(cfg, i)], c_slow[i]);  // (index 0 = <|im_end|>: masked to -inf under FS_GEN_IGNORE_EOS)
        const float worst_slow = worst;
        for (int i = 0; i < a_.codebook_size; ++i) cmp(lf[i], c_fast[i]);
        if (!(worst <= 2e-2f * scale))
            throw Error("self-test \"persist\": persistent kernels disagree with the per-node kernels (max |dlogit| slow " + std::to_string(worst_slow) +
                        ", all " + std::to_string(worst) + " at logit scale " + std::to_string(scale) + "): rebuild with the pinned toolchain or run with FISHRT_NO_PERSIST=1");
    }

    float bench_kernel(int kind, int kv_len, int reps) override {
        use_device();
        require_loaded();
        FS_REQUIRE(kind >= 0 && kind <= 7 && reps >= 1, "bad kernel id");
        FS_REQUIRE(kv_len >= 1 && kv_len < a_.max_seq_len, "bad KV length");
        clear_slow();
        ensure_capacity(0, kv_len);
        SeqState s0 = {};
        s0.pos = kv_len - 1;
        FS_HIP(hipMemcpyAsync(state(0), &s0, sizeof(s0), hipMemcpyHostToDevice, st_));
        set_bucket(kv_len);
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        FS_HIP(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
        int nodes = a_.n_layer;
        if (kind == 5) {  // the fast decoder's layers over the 8 codebook positions (4 nodes per layer)
            for (int cbi = 0; cbi < a_.num_codebooks; ++cbi) enqueue_fast_layers(0, cbi, cbi);
            nodes = a_.num_codebooks * a_.n_fast_layer * 4;
        } else if (kind == 6 || kind == 7) {  // fast / slow (audio-range) head GEMV
            nodes = 16;
            for (int i = 0; i < nodes; ++i) {
                if (kind == 6) LmKernels<WT>::head(d_, xf(0), fast_norm_w_, fast_out_w_, fast_out_s_, a_.codebook_size, d_logits_fast_.as<float>(), st_);
                else LmKernels<WT>::head(d_, x(0), norm_w_, slow_head_w(), slow_head_s(), n_audio_, d_logits_slow_.as<float>(), st_);
            }
        } else
        for (int l = 0; l < a_.n_layer; ++l) {
            const LayerW& w = slow_[l];
            KVView kv = slow_kv(l, 0);
            switch (kind) {
                case 0: LmKernels<WT>::qkv(d_, x(0), w, d_cos_.as<float>(), d_sin_.as<float>(), state(0), 0, 0, d_q_.as<float>(), kv, st_); break;
                case 1: AttnKernels<WT>::decode(d_, d_q_.as<float>(), kv, state(0), d_part_.as<float>(), n_chunks_, nc_launch_, st_); break;
                case 2: LmKernels<WT>::wo(d_, d_part_.as<float>(), n_chunks_, nc_launch_, state(0), nullptr, kv, 0, w, x(0), st_); break;
                case 3: LmKernels<WT>::ffn_up(d_, x(0), w, d_act_.as<float>(), st_); break;
                default: LmKernels<WT>::ffn_down(d_, d_act_.as<float>(), w, x(0), st_); break;
            }
        }
        FS_HIP(hipStreamEndCapture(st_, &g));
        FS_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        FS_HIP(hipGraphDestroy(g));
        FS_HIP(hipGraphLaunch(ge, st_));
        FS_HIP(hipStreamSynchronize(st_));
        FS_HIP(hipEventRecord(ev_[0], st_));
        for (int r = 0; r < reps; ++r) FS_HIP(hipGraphLaunch(ge, st_));
        FS_HIP(hipEventRecord(ev_[1], st_));
        FS_HIP(hipStreamSynchronize(st_));
        float ms = 0.f;
        FS_HIP(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
        (void)hipGraphExecDestroy(ge);
        clear_slow();
        return ms * 1e3f / (float)(reps * nodes);
    }

    // ------------------------------------------------------------------------------------------ generate_blocking
    void generate(const uint32_t* prompt, int L, int max_new_tokens, const fs_sampling& s, uint64_t seed, uint32_t flags,
                  uint32_t* codes_out, size_t cap, size_t* n_frames, fs_frame_cb cb, void* cb_user, float* hidden_out, size_t hidden_cap,
                  size_t* n_hidden) override {
        use_device();
        require_loaded();
        FS_REQUIRE(!sess_active_, "the handle is in session mode (fs_lm_session_end first)");
        const int C = a_.num_codebooks, C1 = C + 1;
        FS_REQUIRE(L >= 1, "empty prompt");
        FS_REQUIRE(max_new_tokens >= 0, "negative max_new_tokens");
        validate_tokens(prompt, (size_t)C1 * L, 1, L);
        const int n_cached = seq_len_[0];
        if (n_cached + L > a_.max_seq_len) throw Error("prompt exceeds max_seq_len (dual_ar.rs:623-624)");
        const Budget budget = iter_budget(max_new_tokens, L, n_cached);
        const long long n_iter = budget.n_iter;
        ensure_capacity(0, n_cached + L + (int)n_iter - 1);
        // device-side setup
        SampleCfg cfg = make_cfg(s, flags);
        cfg.batch_rows = batch_rows_; cfg.batch_row = batch_row_; cfg.batch_calls = a_.num_codebooks + 1;  // batch_rows > 0 only inside generate_batch_sequential
        FS_HIP(hipMemcpyAsync(d_cfg_.p, &cfg, sizeof(cfg), hipMemcpyHostToDevice, st_));
        // greedy decoding on a Fish-geometry bf16 handle: the 8 fast-decoder passes of a frame run as ONE persistent launch
        // (lm_persist.hip) instead of 144 graph nodes, if no other handle of this GPU is using it right now
        std::unique_lock<PersistLock> plock;
        use_persist_ = use_pslow_ = false;
        if ((persist_ok_ || pslow_ok_) && !(flags & FS_GEN_NO_PERSIST)) {
            plock = acquire_persist(device_);
            // the fast kernel decides in-launch: greedily (host ArgMax rule), or with the block-parallel top-k / top-p sampler when top_k <= 256
            persist_sampled_ = cfg.temp != 0.f;
            use_persist_ = plock.owns_lock() && persist_ok_ && batch_rows_ == 0 &&
                           (cfg.temp == 0.f || fast_persist_samples(cfg.temp, cfg.top_k, a_.codebook_size));
            use_pslow_ = plock.owns_lock() && pslow_ok_;                          // the slow kernel feeds any sampler
        }
        // generate_blocking_with_hidden: the slow sampler stores the hidden state of every iteration through this pointer cell
        if (hidden_out && !d_hidden_.p) d_hidden_.alloc(sizeof(float) * (size_t)out_cap_ * a_.dim);
        float* hid_dev = hidden_out ? d_hidden_.as<float>() : nullptr;
        FS_HIP(hipMemcpyAsync(d_hid_slot_.p, &hid_dev, sizeof(hid_dev), hipMemcpyHostToDevice, st_));
        RngState rng;
        upload_rng(seed, rng, d_rng_.as<RngState>(), st_);
        SeqState ss = {};
        ss.pos = n_cached; ss.prompt_L = L;
        FS_HIP(hipMemcpyAsync(state(0), &ss, sizeof(ss), hipMemcpyHostToDevice, st_));
        FS_HIP(hipMemcpyAsync(main_.prompt.p, prompt, sizeof(uint32_t) * C1 * L, hipMemcpyHostToDevice, st_));
        launch_reppen_reset(rp_.view(0), C, a_.codebook_size, st_);
        clear_fast();

        stats_ = {};
        FS_HIP(hipEventRecord(ev_[0], st_));
        // prefill: the first L-1 prompt tokens (MFMA chunks of <= 64 tokens for bf16 weights; sequential token steps for
        // f32 parity handles), then the last prompt token runs as the first frame
        prefill_tokens(0, L - 1, /*use_graph=*/true);
        LmKernels<WT>::embed(d_, tok_emb_, cb_emb_, C, a_.codebook_size, d_cfg_.as<SampleCfg>(), main_.prompt.as<uint32_t>(), state(0),
                             x(0), st_);
        GenRun g;
        g.T0 = n_cached + L; g.n_iter = n_iter; g.cb = cb; g.cb_user = cb_user;
        // FS_GEN_TIME_KERNELS: the frame's two persistent launches one by one, a HIP event in front of / between / behind them
        g.time_k = (flags & FS_GEN_TIME_KERNELS) && use_persist_ && use_pslow_ && fold_slow_sampler();
        if constexpr (std::is_same<WT, bf16_t>::value) {
            if (getenv("FISHRT_B1_ROWS_FAST") && use_persist_ && use_pslow_ && fold_slow_sampler() && !legacy_) {
                ensure_rows(2);
                g.b1_rows_fast = true;
                const int big = 1 << 30;
                FS_HIP(hipMemcpyAsync(d_rcfg_.p, &cfg, sizeof(cfg), hipMemcpyHostToDevice, st_));
                FS_HIP(hipMemcpyAsync(d_rbudget_.p, &big, sizeof(int), hipMemcpyHostToDevice, st_));
                FS_HIP(hipMemcpyAsync(d_rrng_.p, &rng, sizeof(rng), hipMemcpyHostToDevice, st_));
                launch_reppen_reset(rrp_.view(0), C, a_.codebook_size, st_);
            }
        }
        g.multi_ok = use_persist_ && use_pslow_ && fold_slow_sampler() && !g.time_k && !g.b1_rows_fast;
        gen_frame(g, 0);
        FS_HIP(hipEventRecord(ev_[1], st_));
        stats_.graph_launches = (uint64_t)L;
        stats_.kernels_per_frame = (uint64_t)((use_pslow_ ? 1 : a_.n_layer * 5 + 1) + (fold_slow_sampler() ? 0 : 1) +
                                              (use_persist_ ? 1 : a_.num_codebooks * (a_.n_fast_layer * 4 + 2)));
        gen_decode(g);
        SeqState* hs = reinterpret_cast<SeqState*>(h_pin_);  // final state
        FS_HIP(hipEventRecord(ev_[2], st_));
        FS_HIP(hipMemcpyAsync(hs, state(0), sizeof(SeqState), hipMemcpyDeviceToHost, st_));
        FS_HIP(hipStreamSynchronize(st_));
        const size_t n = (size_t)hs->n_out;
        seq_len_[0] = hs->pos;
        float ms01 = 0, ms12 = 0;
        FS_HIP(hipEventElapsedTime(&ms01, ev_[0], ev_[1]));
        FS_HIP(hipEventElapsedTime(&ms12, ev_[1], ev_[2]));
        stats_.prefill_ms = ms01; stats_.decode_ms = ms12; stats_.frames = n; stats_.prompt_tokens = (uint64_t)L;
        if (!g.kev.empty()) {
            double ts = 0, tf = 0;
            for (size_t i = 0; i < g.kev.size(); i += 3) {
                float a = 0, b = 0;
                FS_HIP(hipEventElapsedTime(&a, g.kev[i], g.kev[i + 1]));
                FS_HIP(hipEventElapsedTime(&b, g.kev[i + 1], g.kev[i + 2]));
                ts += a; tf += b;
            }
            stats_.slow_kernel_us = ts * 1e3 / (double)(g.kev.size() / 3);
            stats_.fast_kernel_us = tf * 1e3 / (double)(g.kev.size() / 3);
            for (hipEvent_t e : g.kev) (void)hipEventDestroy(e);
        }
        dump_persist_prof(L);
        if (use_pslow_) check_ctl({&d_sctl_}, "persistent slow-transformer kernel", nullptr);
        if (use_persist_)
            check_ctl({&d_ctl_}, "persistent fast-decoder kernel", "persistent fast-decoder kernel launched with a sampling configuration it was not built for");
        if (budget.clamped && !hs->done && !g.stop)
            throw Error("generation ran past max_seq_len without <|im_end|> (the reference fails at dual_ar.rs:623-624)");
        FS_REQUIRE(n <= cap, "codes_out capacity too small for the generated frames");
        if (codes_out) {
            std::vector<uint32_t> tmp((size_t)C * out_cap_);
            FS_HIP(hipMemcpy(tmp.data(), d_out_.p, sizeof(uint32_t) * C * out_cap_, hipMemcpyDeviceToHost));
            for (int c = 0; c < C; ++c) std::memcpy(codes_out + (size_t)c * cap, tmp.data() + (size_t)c * out_cap_, sizeof(uint32_t) * n);
        }
        if (n_frames) *n_frames = n;
        if (hidden_out) {
            const size_t rows = (size_t)hs->frame;  // iterations executed, the terminating <|im_end|> one included (single_batch.rs:264-266)
            FS_REQUIRE(rows <= hidden_cap, "hidden_out capacity too small for the generator iterations");
            FS_HIP(hipMemcpy(hidden_out, d_hidden_.p, sizeof(float) * rows * a_.dim, hipMemcpyDeviceToHost));
            if (n_hidden) *n_hidden = rows;
        }
    }

    // one generate() call: what its frame launches and its decode loop share
    struct GenRun {
        int T0 = 0;  // KV length of frame 0 (cached + prompt tokens): frame `it` runs at T0 + it
        long long n_iter = 0;
        fs_frame_cb cb = nullptr;
        void* cb_user = nullptr;
        bool time_k = false, b1_rows_fast = false, multi_ok = false;
        std::vector<hipEvent_t> kev;       // FS_GEN_TIME_KERNELS: three events per frame
        long long it = 1;                  // the next generator iteration to enqueue
        size_t delivered = 0;              // frames handed to the callback
        bool stop = false, ended = false;  // the callback asked to stop / the generator has terminated
    };
    // frame `it_` of a generate() call: pick the graph captured for the attention chunk bucket of its KV length
    void gen_frame(GenRun& g, long long it_) {
        set_bucket(g.T0 + (int)it_);
        if (g.b1_rows_fast) {  // experiment hook (FISHRT_B1_ROWS_FAST): the fast decoder of this batch-1 request on k_fast_rows<1>
            launch_slow_persist(pslow_args(), st_);
            RowsFastArgs F = rows_fast_args(0, 1);
            F.slow_logits = d_logits_slow_.as<float>();
            F.cap = nullptr;
            launch_rows_fast(F, 1, persist_sampled_, st_);
            return;
        }
        if (g.time_k && it_ >= 1) {
            for (int i = 0; i < 3; ++i) { hipEvent_t e; FS_HIP(hipEventCreate(&e)); g.kev.push_back(e); }
            FS_HIP(hipEventRecord(g.kev[g.kev.size() - 3], st_));
            launch_slow_persist(pslow_args(), st_);
            FS_HIP(hipEventRecord(g.kev[g.kev.size() - 2], st_));
            launch_fast_persist(persist_args(), persist_sampled_, st_);
            FS_HIP(hipEventRecord(g.kev[g.kev.size() - 1], st_));
            return;
        }
        use_graphs_for_bucket();
        FS_HIP(hipGraphLaunch(g_frame_, st_));
    }
    // decode: one graph replay per frame, enqueued in batches of CHUNK.  Behind every batch the stream copies the generator state
    // and the batch's code columns into pinned memory and records an event; the host looks at batch b (done flag, frame callback)
    // while batch b + 1 is already running, so the GPU never waits for the host between batches
    void gen_decode(GenRun& g) {
        const int C = a_.num_codebooks, CHUNK = g.cb ? 8 : 32;
        auto slot_state = [&](int sl) { return reinterpret_cast<SeqState*>((char*)h_pin_ + 256 + 256 * sl); };
        auto slot_codes = [&](int sl) { return reinterpret_cast<uint32_t*>((char*)h_pin_ + 1024 + 1024 * sl); };  // [C][CHUNK]
        static_assert(sizeof(SeqState) <= 256, "pinned slot size");
        struct Batch { long long first, end; int slot; };
        auto enqueue_batch = [&](int sl) {
            Batch b{g.it, std::min<long long>(g.n_iter, g.it + CHUNK), sl};
            while (g.it < b.end) {
                // several frames per graph launch where the batch has them and they share an attention chunk bucket (multi_frame_graph)
                const int nf = frames_per_graph();
                if (g.multi_ok && nf == 0) {
                    set_bucket(g.T0 + (int)g.it);
                    launch_slow_persist(pslow_args(), st_);
                    launch_fast_persist(persist_args(), persist_sampled_, st_);
                    ++g.it; stats_.graph_launches += 1;
                } else if (g.multi_ok && nf > 1 && b.end - g.it >= nf && chunk_bucket(g.T0 + (int)g.it) == chunk_bucket(g.T0 + (int)g.it + nf - 1)) {
                    set_bucket(g.T0 + (int)g.it);
                    use_graphs_for_bucket();  // (keeps the single-frame graph of the bucket current as well)
                    FS_HIP(hipGraphLaunch(multi_frame_graph(), st_));
                    g.it += nf; stats_.graph_launches += (uint64_t)nf;
                } else {
                    gen_frame(g, g.it); ++g.it; stats_.graph_launches += 1;
                }
            }
            FS_HIP(hipMemcpyAsync(slot_state(sl), state(0), sizeof(SeqState), hipMemcpyDeviceToHost, st_));
            if (g.cb)  // columns [first, end) of every codebook row (frame index == iteration index until <|im_end|>)
                FS_HIP(hipMemcpy2DAsync(slot_codes(sl), sizeof(uint32_t) * CHUNK, d_out_.as<uint32_t>() + b.first, sizeof(uint32_t) * out_cap_,
                                        sizeof(uint32_t) * (size_t)(b.end - b.first), (size_t)C, hipMemcpyDeviceToHost, st_));
            FS_HIP(hipEventRecord(ev_batch_[sl], st_));
            return b;
        };
        auto retire_batch = [&](const Batch& b) {  // the generator's state behind the batch; its frames go to the callback
            FS_HIP(hipEventSynchronize(ev_batch_[b.slot]));
            const SeqState* s2 = slot_state(b.slot);
            if (g.cb) {
                const size_t n = std::min<size_t>((size_t)s2->n_out, (size_t)b.end);
                std::vector<uint32_t> fr(C);
                for (size_t f = std::max<size_t>(g.delivered, (size_t)b.first); f < n && !g.stop; ++f) {
                    for (int c = 0; c < C; ++c) fr[c] = slot_codes(b.slot)[(size_t)c * CHUNK + (f - (size_t)b.first)];
                    if (g.cb(g.cb_user, f, fr.data())) g.stop = true;
                    g.delivered = f + 1;
                }
            }
            if (s2->done != 0) g.ended = true;
        };
        if (g.cb) {  // frame 0 (produced by the prefill iteration) is delivered before the decode batches
            FS_HIP(hipMemcpyAsync(slot_state(0), state(0), sizeof(SeqState), hipMemcpyDeviceToHost, st_));
            FS_HIP(hipMemcpy2DAsync(slot_codes(0), sizeof(uint32_t) * CHUNK, d_out_.as<uint32_t>(), sizeof(uint32_t) * out_cap_, sizeof(uint32_t), (size_t)C,
                                    hipMemcpyDeviceToHost, st_));
            FS_HIP(hipEventRecord(ev_batch_[0], st_));
            retire_batch(Batch{0, 1, 0});
        }
        Batch prev{0, 0, 0};
        bool have_prev = false;
        int sl = g.cb ? 1 : 0;
        while (g.it < g.n_iter && !(g.ended || g.stop)) {
            const Batch cur = enqueue_batch(sl);
            sl ^= 1;
            if (have_prev) retire_batch(prev);  // batch b is examined while batch b + 1 runs
            prev = cur;
            have_prev = true;
        }
        if (have_prev && !g.stop) retire_batch(prev);
    }

    // generate_static_batch (static_batch.rs:282-390).  bf16 / fp8 handles with n <= min(max_batch, kRows): the MFMA row path below
    // (rows = sequences).  Otherwise rows are independent sequences evaluated one after another on KV slot 0 (identical tokens under
    // greedy decoding).  The left padding with <|im_end|>/0 IS applied because the reference never masks it (dual_ar.rs:589-615);
    // repetition penalty is a no-op in the reference's batch path for Fish models (static_batch.rs:204-206 => mask stays 1).
    void generate_batch(const uint32_t* prompts, const int* lens, int n, int max_new_tokens, const fs_sampling& s, uint64_t seed,
                        uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames, uint8_t* is_audio) override {
        FS_REQUIRE(n >= 1, "Must have at least one prompt");  // static_batch.rs:69-71
        FS_REQUIRE(!sess_active_, "the handle is in session mode (fs_lm_session_end first)");
        if (RowKernels<WT>::has_mfma_prefill() && n <= kRows && n <= B_ && a_.dim % 128 == 0 && a_.intermediate_size % 128 == 0 &&
            a_.num_codebooks <= 8 && !legacy_) {
            generate_batch_rows(prompts, lens, n, max_new_tokens, s, seed, flags, codes_out, cap, n_frames, is_audio);
            return;
        }
        generate_batch_sequential(prompts, lens, n, max_new_tokens, s, seed, flags, codes_out, cap, n_frames, is_audio);
    }

    // generate_static_batch on the MFMA row path: the B sequences are the rows of every GEMM (weights streamed once per
    // step for the whole batch), per-row paged KV, per-row on-device sampling, one captured graph per (B, chunk bucket).
    void generate_batch_rows(const uint32_t* prompts, const int* lens, int n, int max_new_tokens, const fs_sampling& s, uint64_t seed,
                             uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames, uint8_t* is_audio) {
        use_device();
        require_loaded();
        const int C = a_.num_codebooks, C1 = C + 1, B = n;
        FS_REQUIRE(t_.has_semantic_end, "static batches need a Fish 1.5 / DualAR token layout (semantic range)");
        int Lmax = 0;
        for (int i = 0; i < n; ++i) { FS_REQUIRE(lens[i] >= 1, "empty prompt"); Lmax = std::max(Lmax, lens[i]); }
        if (Lmax > a_.max_seq_len) throw Error("prompt exceeds max_seq_len (dual_ar.rs:623-624)");
        const Budget budget = iter_budget(max_new_tokens, Lmax);
        const long long n_iter = budget.n_iter;
        clear_slow();  // static_batch.rs:118-121
        clear_fast();
        ensure_prefill_buffers();
        ensure_batch_buffers();
        ensure_rows_capture(B);
        SampleCfg cfg = make_cfg(s, flags);
        cfg.rep_pen = 1.0f;
        rows_par_ = rows_par_sampler_ok(s.temp, s.top_k, n_audio_, a_.codebook_size) && !getenv("FISHRT_ROWS_SAMPLER_1024");
        FS_HIP(hipMemcpyAsync(d_cfg_.p, &cfg, sizeof(cfg), hipMemcpyHostToDevice, st_));
        RngState rng;
        upload_rng(seed, rng, d_rng_.as<RngState>(), st_);  // BatchedLogitsProcessor::new(seed) (the reference passes 42, static_batch.rs:63)
        stats_ = {};
        FS_HIP(hipEventRecord(ev_[0], st_));
        const size_t pstride = (size_t)C1 * Lmax;
        std::vector<uint32_t> padded(pstride * B);
        size_t off = 0;
        for (int b = 0; b < B; ++b) {
            uint32_t* pp = padded.data() + pstride * b;
            left_pad(prompts + off, lens[b], Lmax, pp);
            off += (size_t)C1 * lens[b];
            validate_tokens(pp, pstride, 1, Lmax);
            ensure_capacity(b, Lmax + (int)n_iter - 1);
        }
        const int Lp = Lmax - 1;  // prompt tokens run through the slow transformer before the first frame
        const bool no_group = std::getenv("FISHRT_NO_GROUP_PREFILL") != nullptr;  // test hook: one sequence per pass
        if (Lp >= 1 && Lp <= kRowsCap && a_.head_dim == 64 && !no_group) {
            // group prefill: every prompt has Lmax columns and starts at position 0, so the first Lmax - 1 tokens of as many
            // sequences as fit the row buffers go through ONE pass (GEMM rows = sequences x tokens, flash attention per sequence)
            if (d_bprompt_.n < sizeof(uint32_t) * padded.size()) d_bprompt_.alloc(sizeof(uint32_t) * padded.size());
            FS_HIP(hipMemcpyAsync(d_bprompt_.p, padded.data(), sizeof(uint32_t) * padded.size(), hipMemcpyHostToDevice, st_));
            SeqState ss = {};
            ss.prompt_L = Lmax;
            FS_HIP(hipMemcpyAsync(state(0), &ss, sizeof(ss), hipMemcpyHostToDevice, st_));
            const int per_pass = std::max(1, kRowsCap / Lp);
            for (int b0 = 0; b0 < B; b0 += per_pass)
                launch_group_pass(main_, d_bprompt_.as<uint32_t>() + pstride * b0, std::min(per_pass, B - b0), Lp, pstride, state(0), b0, nullptr, n_chunks_);
            FS_HIP(hipStreamSynchronize(st_));
            for (int b = 0; b < B; ++b) seq_len_[b] = Lp;
        } else {
            for (int b = 0; b < B; ++b) {
                FS_HIP(hipMemcpyAsync(main_.prompt.p, padded.data() + pstride * b, sizeof(uint32_t) * pstride, hipMemcpyHostToDevice, st_));
                SeqState ss = {};
                ss.prompt_L = Lmax;
                FS_HIP(hipMemcpyAsync(state(b), &ss, sizeof(ss), hipMemcpyHostToDevice, st_));
                prefill_tokens(b, Lp, /*use_graph=*/false);
                FS_HIP(hipStreamSynchronize(st_));  // main_.prompt is reused by the next row
                seq_len_[b] = Lp;
            }
        }
        // first-frame inputs: the rows of main_.x are scratch during prefill, so the last prompt column of every row is
        // embedded only now (through the state's `cur` slots)
        for (int b = 0; b < B; ++b) {
            const int L = lens[b];
            SeqState ss = {};
            ss.pos = Lmax - 1; ss.prompt_L = Lmax; ss.step = Lmax - 1;
            const uint32_t* src = prompts;  // find row b's prompt start
            size_t o2 = 0;
            for (int j = 0; j < b; ++j) o2 += (size_t)C1 * lens[j];
            for (int r = 0; r < C1; ++r) ss.cur[r] = src[o2 + (size_t)r * L + (L - 1)];
            FS_HIP(hipMemcpyAsync(state(b), &ss, sizeof(ss), hipMemcpyHostToDevice, st_));
            LmKernels<WT>::embed(d_, tok_emb_, cb_emb_, C, a_.codebook_size, d_cfg_.as<SampleCfg>(), nullptr, state(b),
                                 main_.x.as<float>() + (size_t)b * a_.dim, st_);
            FS_HIP(hipStreamSynchronize(st_));
        }
        auto launch_frame = [&](long long it_) {
            set_bucket(Lmax + (int)it_);
            hipGraphExec_t g = batch_graph(B);
            FS_HIP(hipGraphLaunch(g, st_));
        };
        launch_frame(0);
        FS_HIP(hipEventRecord(ev_[1], st_));
        std::vector<SeqState> hs(B);
        auto all_done = [&]() {
            FS_HIP(hipMemcpyAsync(hs.data(), state(0), sizeof(SeqState) * B, hipMemcpyDeviceToHost, st_));
            FS_HIP(hipStreamSynchronize(st_));
            for (int b = 0; b < B; ++b) if (!hs[b].done) return false;
            return true;
        };
        long long it = 1;
        while (it < n_iter) {
            const long long end = std::min<long long>(n_iter, it + 16);
            for (; it < end; ++it) launch_frame(it);
            if (it < n_iter && all_done()) break;  // prompt = None once every row is dead (:255-258)
        }
        FS_HIP(hipEventRecord(ev_[2], st_));
        const bool done_all = all_done();
        check_rows_xchg();
        float ms01 = 0, ms12 = 0;
        FS_HIP(hipEventElapsedTime(&ms01, ev_[0], ev_[1]));
        FS_HIP(hipEventElapsedTime(&ms12, ev_[1], ev_[2]));
        stats_.prefill_ms = ms01; stats_.decode_ms = ms12; stats_.prompt_tokens = (uint64_t)Lmax * B; stats_.graph_launches = (uint64_t)it;
        if (budget.clamped && !done_all)
            throw Error("generation ran past max_seq_len without <|im_end|> on every row (the reference fails at dual_ar.rs:623-624)");
        stats_.frames = copy_out_rows(hs, B, codes_out, cap, n_frames);
        for (int b = 0; b < B; ++b) {
            // BatchPosition::is_audio (static_batch.rs:229): the first position is returned unconditionally and is not audio when its slow token
            // was <|im_end|> (the row samplers mark that in `step`); every later returned position belongs to a live row, i.e. is a semantic token
            if (is_audio)
                for (size_t f = 0; f < n_frames[b]; ++f) is_audio[(size_t)b * cap + f] = (f == 0 && hs[b].step == -1) ? 0 : 1;
        }
    }

    // ---- continuous batching: the rows of the static-batch step as independent request slots.  No reference counterpart (the reference
    // serialises requests behind one mutex, server/lib/state.rs:12-29, or runs lock-step static batches, static_batch.rs:282-390); a slot
    // behaves exactly like row 0 of a one-prompt generate_static_batch: no left padding (its own positions / KV pages), first frame
    // emitted unconditionally, BatchedLogitsProcessor sampling, no repetition penalty, 1 + max(0, max_new_tokens - L + 1) iterations.
    // Requests join between steps (their prompt is prefilled on the row path while the other slots wait) and leave when done.
    void session_begin(const fs_sampling& s, uint64_t seed, uint32_t flags) override {
        use_device();
        require_loaded();
        FS_REQUIRE(!sess_active_, "a session is already open on this handle");
        FS_REQUIRE(RowKernels<WT>::has_mfma_prefill() && B_ <= kRows && a_.dim % 128 == 0 && a_.intermediate_size % 128 == 0 && a_.num_codebooks <= 8,
                   "sessions need the MFMA row path (bf16 / fp8 handle)");
        // FS_SESSION_SCORE: the step graphs of the session carry one score node in front of each per-slot sampler node (k_score_slots);
        // slots admitted with fs_lm_session_add_scored are forced through them, every other slot is untouched
        const bool score = (flags & FS_SESSION_SCORE) != 0;
        if (score) {
            if (flags & FS_SESSION_ROWS) throw Error("FS_SESSION_SCORE is valid only together with FS_SESSION_PER_SLOT: not with FS_SESSION_ROWS");
            if (!(flags & FS_SESSION_PER_SLOT)) throw Error("FS_SESSION_SCORE is valid only together with FS_SESSION_PER_SLOT: not alone");
            if (legacy_ || !t_.has_semantic_end)
                throw Error("FS_SESSION_SCORE needs the Fish 1.5 token layout (has_semantic_end != 0): a Fish <= 1.4 handle has no slow-token distribution to score");
            FS_REQUIRE(a_.num_codebooks == 8, "FS_SESSION_SCORE needs num_codebooks == 8 (the score record holds 9 decisions per iteration)");
        }
        // FS_SESSION_TRACE: the score nodes of the session also serve TRACED slots (fs_lm_session_add_traced: they sample, and leave the
        // scoring slots' record of their own picks), and one tail node behind the frame's last sampler closes their rows (k_trace_commit)
        const bool trace = (flags & FS_SESSION_TRACE) != 0;
        if (trace) {
            if (flags & FS_SESSION_ROWS) throw Error("FS_SESSION_TRACE is valid only together with FS_SESSION_PER_SLOT | FS_SESSION_SCORE: not with FS_SESSION_ROWS");
            if (!(flags & FS_SESSION_PER_SLOT)) throw Error("FS_SESSION_TRACE is valid only together with FS_SESSION_PER_SLOT | FS_SESSION_SCORE: not alone");
            if (!score) throw Error("FS_SESSION_TRACE is valid only together with FS_SESSION_PER_SLOT | FS_SESSION_SCORE: not without FS_SESSION_SCORE");
        }
        // FS_SESSION_ALTS: the score nodes of the session are the instantiation that also leaves the N most likely candidates and the entropy
        // of every decision of a scoring or traced slot (fs_lm_session_poll_alts); N = the FS_SESSION_ALTS_N field of the flags, 0 = 8
        const uint32_t alts_field = (flags >> 16) & 31u;
        int alts_n = 0;
        if (flags & FS_SESSION_ALTS) {
            if (flags & FS_SESSION_ROWS) throw Error("FS_SESSION_ALTS is valid only together with FS_SESSION_PER_SLOT | FS_SESSION_SCORE: not with FS_SESSION_ROWS");
            if (!(flags & FS_SESSION_PER_SLOT)) throw Error("FS_SESSION_ALTS is valid only together with FS_SESSION_PER_SLOT | FS_SESSION_SCORE: not alone");
            if (!score) throw Error("FS_SESSION_ALTS is valid only together with FS_SESSION_PER_SLOT | FS_SESSION_SCORE: not without FS_SESSION_SCORE");
            if (alts_field > FS_ALTS_MAX)
                throw Error("FS_SESSION_ALTS_N(" + std::to_string(alts_field) + ") exceeds FS_ALTS_MAX (16): a decision records 1 .. 16 alternatives (0 = the default of 8)");
            alts_n = alts_field ? (int)alts_field : 8;
        } else if (alts_field) {
            throw Error("FS_SESSION_ALTS_N(" + std::to_string(alts_field) + ") without FS_SESSION_ALTS: the field is read only together with the flag");
        }
        // Fish <= 1.4 handles (no semantic range: the slow token is the 2-way {pad, im_end} draw): only the per-slot samplers define that
        // decision for a slot (k_sample_slow_slots, as the slot's own fs_lm_generate call); the lock-step sampler and the request-row
        // kernels do not
        FS_REQUIRE((!legacy_ && t_.has_semantic_end) || ((flags & FS_SESSION_PER_SLOT) && !(flags & FS_SESSION_ROWS)),
                   "plain and FS_SESSION_ROWS sessions need the Fish 1.5 token layout; Fish <= 1.4 handles take FS_SESSION_PER_SLOT");
        clear_slow();
        clear_fast();
        ensure_prefill_buffers();
        ensure_batch_buffers();
        // FS_SESSION_ROWS: the slots run on the request-row persistent kernels (lm_persist_rows.hip) and keep BATCH-1 semantics -- every slot is
        // its own generate_blocking (repetition penalty, its own LogitsProcessor stream seeded seed + its admission number) -- instead of the
        // static-batch sampler's.  Needs max_batch <= 8, a bf16 Fish-1.5 handle and a sampler setting the in-launch decisions cover.
        // The mode is built in a local and becomes the handle's with sess_active_, as the last act: a throw leaves the handle as it was.
        SessMode m;
        m.score = score; m.trace = trace; m.alts = alts_n;
        // FS_SESSION_PER_SLOT: the slots stay on the static-batch step, but its 9 sampler nodes are the per-slot ones (k_sample_*_slots):
        // every slot decides like its own generate_blocking call, with its own settings, StdRng stream and repetition-penalty windows
        m.slots = (flags & FS_SESSION_PER_SLOT) != 0;
        // FS_SESSION_WIDE_SAMPLER: the per-slot sampler nodes are the instantiation that also covers nucleus-only and top_k > 256 settings
        m.wide = (flags & FS_SESSION_WIDE_SAMPLER) != 0;
        FS_REQUIRE(!m.wide || (m.slots && !(flags & FS_SESSION_ROWS)),
                   "FS_SESSION_WIDE_SAMPLER is valid only together with FS_SESSION_PER_SLOT (not alone, not with FS_SESSION_ROWS)");
        FS_REQUIRE(!(m.slots && (flags & FS_SESSION_ROWS)), "FS_SESSION_PER_SLOT and FS_SESSION_ROWS exclude each other (a row session's slots already sample per slot)");
        if (m.slots) {
            FS_REQUIRE(n_audio_ <= 2048 && a_.codebook_size <= 1024, "FS_SESSION_PER_SLOT needs <= 2048 slow candidates and codebooks of <= 1024 entries");
            require_slot_sampling(s, m.wide);
        }
        std::unique_lock<PersistLock> rows_lock;  // (a local: anything thrown below releases it)
        if (flags & FS_SESSION_ROWS) {
            const char* why = nullptr;
            if (!rows_predicate(B_, &s, 1, /*for_session=*/true, &why)) throw Error(std::string("FS_SESSION_ROWS needs ") + why);
            FS_REQUIRE(pages_.free_count() > 0, "KV page pool exhausted");  // (the scratch page below: nothing may throw once the lock is held)
            // the device's persistent-kernel lock is held in a LOCAL until nothing below can throw any more (a throw after taking it used to
            // leave sess_plock_ owning the mutex with sess_active_ false: session_end returned early and the device was locked out for good)
            rows_lock = acquire_persist(device_);
            FS_REQUIRE(rows_lock.owns_lock(), "another call on this device holds the persistent kernels");
            ensure_rows(B_);
            m.rows = true;
            m.R = B_;
            m.sampled = s.temp != 0.0;
        }
        sess_seed_ = seed;
        sess_adds_ = 0;
        ensure_rows_capture(B_);
        SampleCfg cfg = make_cfg(s, flags);
        if (!m.rows && !m.slots) cfg.rep_pen = 1.0f;
        cfg.session = m.rows ? 0 : 1;
        sess_cfg_ = cfg;
        if (m.slots) {
            // per-slot sampler state, allocated once per handle (the captured step graphs hold these pointers) and re-initialised for every
            // slot at its activation, so nothing of an earlier session or occupant is ever read
            if (!d_scfg_.p) {
                d_scfg_.alloc(sizeof(SampleCfg) * B_);
                d_srng_.alloc(sizeof(SlotRng) * B_);
                srp_.alloc(B_, a_.num_codebooks, a_.codebook_size);
            }
            std::vector<SampleCfg> cfgs(B_, cfg);
            FS_HIP(hipMemcpyAsync(d_scfg_.p, cfgs.data(), sizeof(SampleCfg) * B_, hipMemcpyHostToDevice, st_));
            FS_HIP(hipMemsetAsync(d_srng_.p, 0xFF, d_srng_.n, st_));
            FS_HIP(hipMemsetAsync(srp_.ring.p, 0, srp_.ring.n, st_));
            for (int b = 0; b < B_; ++b) launch_reppen_reset(srp_.view(b), a_.num_codebooks, a_.codebook_size, st_);
            FS_HIP(hipStreamSynchronize(st_));  // (cfgs is a local)
        }
        if (m.rows) {
            std::vector<SampleCfg> cfgs(m.R, cfg);
            FS_HIP(hipMemcpyAsync(d_rcfg_.p, cfgs.data(), sizeof(SampleCfg) * m.R, hipMemcpyHostToDevice, st_));
            float* nullp = nullptr;
            FS_HIP(hipMemcpyAsync(d_hid_slot_.p, &nullp, sizeof(nullp), hipMemcpyHostToDevice, st_));
            FS_HIP(hipStreamSynchronize(st_));  // (cfgs is a local)
        }
        rows_par_ = !m.slots && rows_par_sampler_ok(s.temp, s.top_k, n_audio_, a_.codebook_size) && !getenv("FISHRT_ROWS_SAMPLER_1024");
        FS_HIP(hipMemcpyAsync(d_cfg_.p, &cfg, sizeof(cfg), hipMemcpyHostToDevice, st_));
        RngState rng;
        upload_rng(seed, rng, d_rng_.as<RngState>(), st_);
        // empty slots: dead, frame 1 (so the frame-0 rule never fires), position 0 of a scratch page nobody reads
        sess_scratch_ = pages_.hold_new();
        sess_left_.assign(B_, kSlotFree);
        sess_pos_.assign(B_, 0);
        sess_L_.assign(B_, 0);
        sess_hs_.assign(B_, SeqState{});
        sess_queue_.clear(); sess_flight_.clear();
        sess_prefixes_.clear();
        tab_begin(hid_, sizeof(float) * (size_t)a_.dim);
        // (the book frees its pool when the row size differs from the previous session's: FS_SESSION_ALTS rows are longer, by N)
        tab_begin(sc_, sizeof(float) * SCORE_REC_WORDS + sizeof(uint32_t) * ((size_t)a_.num_codebooks + 1) +
                           (alts_n ? score_alts_bytes(a_.num_codebooks + 1, alts_n) : 0));
        sess_traced_.assign(B_, 0);
        if (trace) {
            // the traced slots' stash, allocated once per handle (the captured step graphs of trace sessions hold its address); no row is open
            if (!d_trace_.p) d_trace_.alloc(sizeof(float) * (size_t)B_ * TRACE_STASH_WORDS);
            FS_HIP(hipMemsetAsync(d_trace_.p, 0, d_trace_.n, st_));
        }
        for (auto& v : sess_count_) v = 0;
        sess_pf_ms_ = 0.0;
        sess_timed_ = false;
        for (int b = 0; b < B_; ++b) park_slot(b, m.rows);
        FS_HIP(hipMemsetAsync(main_.x.p, 0, sizeof(float) * (size_t)B_ * a_.dim, st_));
        FS_HIP(hipStreamSynchronize(st_));
        stats_ = {};
        if (m.rows) sess_plock_ = std::move(rows_lock);
        sess_ = m;
        sess_active_ = true;
    }
    // what a slot of a FS_SESSION_PER_SLOT session may sample with: the boundary of the in-launch samplers (fishrt.h: fs_lm_generate)
    // In a wide session (FS_SESSION_WIDE_SAMPLER): greedy, or temp > 0 with any top_k and any finite top_p.
    void require_slot_sampling(const fs_sampling& s, bool wide) const {
        if (const char* e = slot_sampling_error(s.temp, s.top_p, s.top_k, wide)) throw Error(e);
    }
    // the states of a slot, as sess_left_ spells them (>= 0: iterations left to a live slot), and the check of the entry points that take one
    static constexpr int kSlotFree = -1, kSlotPrefilling = -2;
    bool slot_free(int b) const { return sess_left_[b] == kSlotFree; }
    bool slot_prefilling(int b) const { return sess_left_[b] == kSlotPrefilling; }
    bool slot_running(int b) const { return sess_left_[b] > 0 && !sess_hs_[b].done; }
    void require_live_slot(int slot) const { FS_REQUIRE(sess_active_ && slot >= 0 && slot < B_ && !slot_free(slot), "not a live session slot"); }
    // Admission of a slot, whichever entry point asked (fishrt.h: fs_lm_session_add / _add_prefixed / _add_ex / _add_hidden / _add_scored /
    // _add_traced; SlotRequest), to the lowest free slot: -1 when none is free or the KV page pool is short right now -- pages come back
    // when slots are released -- neither is an error.  One path, straight down: the request is validated in full, then the slot and the
    // pool are looked at, and only a request that will be admitted takes anything (collector buffers, pages) and is QUEUED, complete, in
    // one push.  A plain add is a prefixed add with an empty prefix (P = 0, no shared pages, no tail); a prefixed one is the add of
    // concat(prefix, body) except that the slot's page table starts with the prefix's full pages (shared), only the body is prefilled
    // and the slot reserves its private pages only.
    // Settings / seed of its own: per-slot sessions take anything inside require_slot_sampling; row sessions what their launch
    // instantiation covers together with the session's setting (all greedy or all sampled); the lock-step sampler has no per-slot
    // notion, so a plain session refuses both.
    // Collectors: a hidden-state slot gets a row buffer, a scoring or traced slot a record buffer (records [cap][32] f32, then [cap][C + 1]
    // u32: a scoring slot's targets, a traced slot's token rows), one row per iteration the slot can run; they travel in hand with the
    // PendingAdd and the device tables learn of them at activation, so the slot's rows start at 0 with its first iteration.
    // A scoring slot (r.frames [C + 1][N]) is forced through exactly N iterations and scored (k_score_slots in front of each of the step's
    // sampler nodes): its SampleCfg is the session's made greedy with no repetition penalty, so its sampler nodes pick the +INFINITY
    // the score node leaves at the target.  Scoring and traced slots always carry a seed of their own -- the one they would have had
    // anyway when the caller gives none -- which gives them a prefill pass of their own (flush_pending), so their records are a function
    // of the request alone (a scoring slot draws no word).
    int session_admit(const SlotRequest& r) override {
        use_device();
        // 1. whatever makes the request a bad one, before anything is taken or changed
        FS_REQUIRE(sess_active_, "no open session");
        const bool scored = r.frames != nullptr, prefixed = r.prefix_id >= 0;
        FS_REQUIRE(!scored || sess_.score, "fs_lm_session_add_scored needs FS_SESSION_SCORE (begin the session with FS_SESSION_PER_SLOT | FS_SESSION_SCORE)");
        FS_REQUIRE(!r.traced || sess_.trace, "fs_lm_session_add_traced needs FS_SESSION_TRACE (begin the session with FS_SESSION_PER_SLOT | FS_SESSION_SCORE | FS_SESSION_TRACE)");
        FS_REQUIRE(r.L >= 1, prefixed ? "empty body (a prefixed add needs its last prompt column)" : "empty prompt");
        const int C1 = a_.num_codebooks + 1, N = r.N;
        if (scored) {
            FS_REQUIRE(N >= 1, "frames: N must be >= 1");
            for (int i = 0; i < N; ++i) {
                const uint32_t tok = r.frames[i];
                if (tok < t_.semantic_start_id || tok >= (uint32_t)a_.vocab_size)
                    throw Error("frames[0][" + std::to_string(i) + "] = " + std::to_string(tok) + ": a forced slow token must lie in [semantic_start_id, vocab_size) "
                                "(<|im_end|> and text tokens cannot be scored as a frame)");
                for (int c = 1; c < C1; ++c)
                    if (r.frames[(size_t)c * N + i] >= (uint32_t)a_.codebook_size)
                        throw Error("frames[" + std::to_string(c) + "][" + std::to_string(i) + "] = " + std::to_string(r.frames[(size_t)c * N + i]) + ": a code must be < codebook_size");
            }
        }
        const int P = prefixed ? live_prefix(r.prefix_id).P : 0;
        const long long Lt = (long long)P + r.L;
        if (scored && Lt + N - 1 > a_.max_seq_len)
            throw Error("L + N - 1 = " + std::to_string(Lt + N - 1) + " exceeds max_seq_len (L counts the prefix; a scored sequence is never clipped)");
        if (r.sampling || r.seed) {
            if (!sess_.slots && !sess_.rows)
                throw Error("per-slot sampling / seed need a session begun with FS_SESSION_PER_SLOT or FS_SESSION_ROWS (the lock-step sampler has one setting and one stream per session)");
            if (r.sampling && sess_.slots) require_slot_sampling(*r.sampling, sess_.wide);
            if (r.sampling && sess_.rows) {
                if ((r.sampling->temp != 0.0) != sess_.sampled) throw Error("FS_SESSION_ROWS: every slot greedy or every slot sampled, like the session's own setting");
                if (sess_.sampled && !fast_persist_samples((float)r.sampling->temp, clamp_top_k(r.sampling->top_k), a_.codebook_size))
                    throw Error("FS_SESSION_ROWS: sampled slots need temp > 0 and 0 < top_k <= 256");
            }
        }
        if (Lt > a_.max_seq_len) throw Error("prompt exceeds max_seq_len (dual_ar.rs:623-624)");
        validate_tokens(r.prompt, 0, 1, r.L);
        // the slot's iterations, computed once: a slot stops at max_seq_len instead of erroring; a scored one runs exactly N (never clipped)
        const int L = (int)Lt, n_iter = (int)iter_budget(scored ? Lt + N - 2 : r.max_new_tokens, Lt).n_iter;
        FS_REQUIRE(!scored || n_iter == N, "score buffer shorter than the slot's iterations");
        // 2. room right now?  (reads only)
        int b = -1;
        for (int i = 0; i < B_; ++i) if (slot_free(i)) { b = i; break; }
        if (b < 0) return -1;
        const int nfull = P / KV_PAGE, end = L + n_iter - 1;  // the prefix's full pages are shared; positions < end keep their K/V
        const KvPages::Share shared{prefixed ? pages_.prefix_owner(r.prefix_id) : -1, nfull};
        if (!pages_.room(b, end, shared).fits) return -1;  // (a free slot that still holds pages is an error, raised here)
        ensure_join_lane();
        // 3. the queue entry, complete but for what is taken below
        PendingAdd pa;
        pa.slot = pa.owner = b; pa.L = L; pa.n_iter = n_iter; pa.start = P; pa.prefix = r.prefix_id; pa.traced = r.traced;
        pa.prompt.assign(r.prompt, r.prompt + (size_t)C1 * r.L);
        pa.has_seed = r.seed || scored || r.traced;
        pa.seed = r.seed ? *r.seed : sess_seed_ + (uint64_t)sess_adds_;
        if (scored) {
            pa.has_cfg = true;
            pa.cfg = sess_cfg_;
            pa.cfg.temp = 0.f; pa.cfg.rep_pen = 1.f;
            pa.sc_targets.resize((size_t)N * C1);  // [N][C + 1]: one iteration's 9 targets side by side
            for (int i = 0; i < N; ++i)
                for (int c = 0; c < C1; ++c) pa.sc_targets[(size_t)i * C1 + c] = r.frames[(size_t)c * N + i];
        } else if (r.sampling) {  // the session's SampleCfg with this request's settings
            pa.has_cfg = true;
            pa.cfg = make_cfg(*r.sampling, sess_cfg_.ignore_eos ? FS_GEN_IGNORE_EOS : 0);
            pa.cfg.session = sess_cfg_.session;
        }
        // 4. the collector buffers, the first thing taken (an allocation failure leaves the session as it was)
        if (r.collect_hidden) pa.hid = hid_.book.take(n_iter);
        if (scored || r.traced) {
            try { pa.sc = sc_.book.take(n_iter); } catch (...) { hid_.book.put(pa.hid); throw; }
        }
        // 5. the pages: references on the prefix's full ones, the slot's private ones, and a hold on the prefix's partly filled last page
        // until it has been copied.  None of the three can fail: the room query of step 2 asked for exactly this, and nothing has touched
        // the book since.  (No upload: the row of a parked slot keeps pointing at the scratch page until activate_pending.)
        pages_.share(b, shared);
        pages_.grow(b, end);
        if (P % KV_PAGE) pa.tail = pages_.hold_page_of(shared.from, nfull);
        // 6. queued: the slot is reserved, and polls of its collectors are answered from now on
        pa.order = sess_adds_++;
        sess_queue_.push_back(std::move(pa));
        sess_left_[b] = kSlotPrefilling;
        if (r.collect_hidden) hid_.book.admitted(b);
        if (scored || r.traced) sc_.book.admitted(b);
        sess_traced_[b] = r.traced ? 1 : 0;
        stats_.prompt_tokens += (uint64_t)L;
        return b;
    }
    // What a collector table (hid_, sc_) does on the device side of the book's moves.  Session begin / end: a null device table.  Activation:
    // the slot's entry, count 0 (it collects from its first iteration on: row 0).  Drop: the slot stops collecting -- null entry on the
    // engine stream, ahead of the next step.  End of a chunk: the device table comes back and, once the stream has been waited for, the
    // book takes its counts.
    template <typename E> void tab_begin(SlotTab<E>& t, size_t row_bytes) { t.book.begin(B_, row_bytes); tab_clear(t); }
    template <typename E> void tab_end(SlotTab<E>& t) { t.book.end(); tab_clear(t); }
    template <typename E> void tab_clear(SlotTab<E>& t) { FS_HIP(hipMemsetAsync(t.dev.p, 0, t.dev.n, st_)); }
    template <typename E> void tab_upload(SlotTab<E>& t, int b) { FS_HIP(hipMemcpyAsync(t.dev.template as<E>() + b, &t.book.entry(b), sizeof(E), hipMemcpyHostToDevice, st_)); }
    template <typename E> void tab_activate(SlotTab<E>& t, int b, const SlotBuf& buf) { t.book.activate(b, buf); tab_upload(t, b); }
    template <typename E> void tab_drop(SlotTab<E>& t, int b) {
        if (!t.book.drop(b)) return;
        tab_upload(t, b);
        FS_HIP(hipStreamSynchronize(st_));
    }
    template <typename E> void tab_fetch_counts(SlotTab<E>& t) {
        t.stage.resize(B_);
        if (t.book.live() > 0) FS_HIP(hipMemcpyAsync(t.stage.data(), t.dev.p, sizeof(E) * B_, hipMemcpyDeviceToHost, st_));
    }
    template <typename E> void tab_take_counts(SlotTab<E>& t) { if (t.book.live() > 0) t.book.refresh_counts(t.stage.data()); }
    void session_poll_hidden(int slot, size_t first_row, float* hidden_out, size_t cap_rows, size_t* n_rows) override {
        use_device();
        require_live_slot(slot);
        FS_REQUIRE(hid_.book.wanted(slot), "the slot does not collect hidden states (it was not admitted with fs_lm_session_add_hidden)");
        const HidSlot& e = hid_.book.entry(slot);
        const size_t n = slot_prefilling(slot) ? 0 : (size_t)e.count;
        if (hidden_out && first_row < n) {
            const size_t m = std::min(n - first_row, cap_rows);
            if (m) FS_HIP(hipMemcpyAsync(hidden_out, e.rows + first_row * (size_t)a_.dim, sizeof(float) * m * a_.dim, hipMemcpyDeviceToHost, st_));
            FS_HIP(hipStreamSynchronize(st_));
        }
        if (n_rows) *n_rows = n;
    }
    // the records [first_row, rows so far) of a scoring or traced slot, unpacked into whichever outputs are given ([n][C + 1] per decision,
    // [n] per iteration); tokens / n_decisions: the rows behind the records, a traced slot's picks.  *n_rows = rows so far.
    struct RecordsOut {
        float *logprob, *top_logprob;
        uint32_t* top;
        float* eos_logprob;
        uint32_t* tokens = nullptr;
        int* n_decisions = nullptr;
    };
    void poll_records(int slot, size_t first_row, size_t cap_rows, const RecordsOut& o, size_t* n_rows) {
        const ScoreSlot& e = sc_.book.entry(slot);
        const size_t n = slot_prefilling(slot) ? 0 : (size_t)e.count;
        const bool want_tokens = o.tokens || o.n_decisions;
        if ((o.logprob || o.top_logprob || o.top || o.eos_logprob || want_tokens) && first_row < n) {
            const size_t m = std::min(n - first_row, cap_rows), C1 = (size_t)a_.num_codebooks + 1;
            std::vector<float> rec(m * SCORE_REC_WORDS);
            std::vector<uint32_t> tk(want_tokens ? m * C1 : 0);
            if (m) FS_HIP(hipMemcpyAsync(rec.data(), e.rec + first_row * SCORE_REC_WORDS, sizeof(float) * rec.size(), hipMemcpyDeviceToHost, st_));
            if (m && want_tokens) FS_HIP(hipMemcpyAsync(tk.data(), e.targets + first_row * C1, sizeof(uint32_t) * tk.size(), hipMemcpyDeviceToHost, st_));
            FS_HIP(hipStreamSynchronize(st_));
            for (size_t i = 0; i < m; ++i) {
                const float* r = rec.data() + i * SCORE_REC_WORDS;
                for (size_t d = 0; d < C1; ++d) {
                    if (o.tokens) o.tokens[i * C1 + d] = tk[i * C1 + d];
                    if (o.logprob) o.logprob[i * C1 + d] = r[SCORE_REC_LOGPROB + d];
                    if (o.top_logprob) o.top_logprob[i * C1 + d] = r[SCORE_REC_TOP_LOGPROB + d];
                    if (o.top) std::memcpy(&o.top[i * C1 + d], &r[SCORE_REC_TOP + d], sizeof(uint32_t));
                }
                if (o.eos_logprob) o.eos_logprob[i] = r[SCORE_REC_EOS];
                // (an iteration whose slow pick was <|im_end|> made that one decision; tokens[.][0] is then <|im_end|>'s id)
                if (o.n_decisions) o.n_decisions[i] = tk[i * C1] == t_.im_end_id ? 1 : (int)C1;
            }
        }
        if (n_rows) *n_rows = n;
    }
    void session_poll_scores(int slot, size_t first_row, float* logprob, float* top_logprob, uint32_t* top, float* eos_logprob, size_t cap_rows,
                             size_t* n_rows) override {
        use_device();
        FS_REQUIRE(sess_active_, "no open session");
        FS_REQUIRE(sess_.score, "fs_lm_session_poll_scores needs FS_SESSION_SCORE (begin the session with FS_SESSION_PER_SLOT | FS_SESSION_SCORE)");
        require_live_slot(slot);
        FS_REQUIRE(sc_.book.wanted(slot) && !sess_traced_[slot], "the slot is not a scoring slot (it was not admitted with fs_lm_session_add_scored)");
        poll_records(slot, first_row, cap_rows, RecordsOut{logprob, top_logprob, top, eos_logprob}, n_rows);
    }
    void session_poll_trace(int slot, size_t first_row, uint32_t* tokens, float* logprob, float* top_logprob, uint32_t* top, float* eos_logprob,
                            int* n_decisions, size_t cap_rows, size_t* n_rows) override {
        use_device();
        FS_REQUIRE(sess_active_, "no open session");
        FS_REQUIRE(sess_.trace, "fs_lm_session_poll_trace needs FS_SESSION_TRACE (begin the session with FS_SESSION_PER_SLOT | FS_SESSION_SCORE | FS_SESSION_TRACE)");
        require_live_slot(slot);
        FS_REQUIRE(sc_.book.wanted(slot) && sess_traced_[slot], "the slot is not a traced slot (it was not admitted with fs_lm_session_add_traced)");
        poll_records(slot, first_row, cap_rows, RecordsOut{logprob, top_logprob, top, eos_logprob, tokens, n_decisions}, n_rows);
    }
    // the alternatives [first_row, rows so far) of a scoring or traced slot of a FS_SESSION_ALTS session: the three blocks behind the slot's
    // records and targets / token rows, [n][C + 1][N] / [n][C + 1] as they lie on the device
    void session_poll_alts(int slot, size_t first_row, uint32_t* alt_index, float* alt_logprob, float* entropy, size_t cap_rows, size_t* n_rows,
                           int* n_alts) override {
        use_device();
        FS_REQUIRE(sess_active_, "no open session");
        FS_REQUIRE(sess_.alts > 0, "fs_lm_session_poll_alts needs FS_SESSION_ALTS (begin the session with FS_SESSION_PER_SLOT | FS_SESSION_SCORE | FS_SESSION_ALTS)");
        require_live_slot(slot);
        FS_REQUIRE(sc_.book.wanted(slot), "the slot is neither a scoring nor a traced slot (it was not admitted with fs_lm_session_add_scored / _add_traced)");
        const ScoreSlot& e = sc_.book.entry(slot);
        const size_t n = slot_prefilling(slot) ? 0 : (size_t)e.count;
        if ((alt_index || alt_logprob || entropy) && first_row < n) {
            const size_t m = std::min(n - first_row, cap_rows), C1 = (size_t)a_.num_codebooks + 1, N = (size_t)sess_.alts;
            if (m && alt_index)
                FS_HIP(hipMemcpyAsync(alt_index, score_alt_index(e, (int)C1) + first_row * C1 * N, sizeof(uint32_t) * m * C1 * N, hipMemcpyDeviceToHost, st_));
            if (m && alt_logprob)
                FS_HIP(hipMemcpyAsync(alt_logprob, score_alt_logprob(e, (int)C1, (int)N) + first_row * C1 * N, sizeof(float) * m * C1 * N, hipMemcpyDeviceToHost, st_));
            if (m && entropy)
                FS_HIP(hipMemcpyAsync(entropy, score_alt_entropy(e, (int)C1, (int)N) + first_row * C1, sizeof(float) * m * C1, hipMemcpyDeviceToHost, st_));
            FS_HIP(hipStreamSynchronize(st_));
        }
        if (n_rows) *n_rows = n;
        if (n_alts) *n_alts = sess_.alts;
    }
    void park_slot(int b, bool rows) {
        SeqState ss = {};
        ss.done = rows ? 2 : 1; ss.frame = 1;  // (rows mode: a terminated row is skipped by the row kernels altogether)
        sess_hs_[b] = ss;
        FS_HIP(hipMemcpyAsync(state(b), &sess_hs_[b], sizeof(SeqState), hipMemcpyHostToDevice, st_));
        upload_row(b, st_, &sess_scratch_, 1);
        FS_HIP(hipStreamSynchronize(st_));
    }
    // Joining requests are prefilled on a second stream with their own row buffers, staging SeqState (index B_) and page-table rows
    // (B_ ..), so the decode steps of the live slots go on underneath; a joining slot stays parked (scratch page, frozen) until its prefill
    // has finished and activate_pending() -- between two steps -- hands it its page-table row, state and first input embedding.
    // session_admit only QUEUES the request; flush_pending() (first thing in session_step, or when the row buffers are full) prefills
    // everything queued as GROUP passes: requests sorted by length, each pass = as many of them as fit the 2048 activation rows,
    // right-padded to the longest of the pass (rows = sequences x tokens, RowMap.seq_rows; causal attention: a real token never sees a
    // pad token, and the K/V a pad position writes into the slot's own pages lies beyond its length, where the first decode steps
    // overwrite it before anything reads it).  A burst of 32 requests is admitted in 2-3 passes instead of 32.
    // a queued request: plain add (prompt = all L columns, start 0), prefixed add (prompt = the body's L - start columns, start = the
    // prefix's P, tail = the prefix's partly filled last page, held until the copy has run) or a prefix's own pass (create: prompt = its P
    // columns, all of them prefilled into the prefix's pages; slot -1) or a prefix's import (create and import_kv: blob = the payload of
    // fs_lm_session_prefix_import, copied and scattered into the prefix's pages; no prompt, nothing runs through the slow transformer)
    // What the choice of a pass reads of it is its PrefillMember (fs_prefill_plan.h: L, n_iter, start, create, import_kv, has_seed -- a
    // sampler seed of its own, fs_lm_session_add_ex -- and owner, whose pages its pass writes: the slot, or the prefix being created).
    struct PendingAdd : PrefillMember {
        int slot = -1, order = 0, prefix = -1, tail = -1;
        std::vector<uint8_t> blob;
        bool has_cfg = false;  // fs_lm_session_add_ex: the slot's own settings
        SampleCfg cfg = {};
        uint64_t seed = 0;
        SlotBuf hid;                       // fs_lm_session_add_hidden: the slot's row buffer [cap][dim], handed to the device table at activation
        SlotBuf sc;                        // fs_lm_session_add_scored: the slot's records + targets buffer, likewise (both in hand until then)
        std::vector<uint32_t> sc_targets;  // ... and the staged targets [n_iter][C + 1], copied into the buffer then
        bool traced = false;               // fs_lm_session_add_traced: `sc` is the slot's records + token rows; its table entry has no targets
        std::vector<uint32_t> prompt;      // [C + 1][cols()]
    };
    // a session's shared prefix; its pages are those of owner pages_.prefix_owner(id) (one reference each, held until released or the
    // session ends; slots add their own on the full ones).  pending: its own pass has still to be activated (a release then waits for that)
    struct SessPrefix { int P = 0; bool live = false, pending = false; };
    // Shared conditioning prefixes (fishrt.h: fs_lm_session_prefix_create).  The prefix is queued like an add; its pages are taken now,
    // so the pool check stays cumulative over everything admitted since.
    int session_prefix_create(const uint32_t* prompt, int P) override {
        use_device();
        FS_REQUIRE(sess_active_, "no open session");
        FS_REQUIRE(P >= 1, "empty prefix");
        FS_REQUIRE(P < a_.max_seq_len, "prefix leaves no room for a body within max_seq_len");
        validate_tokens(prompt, 0, 1, P);
        PendingAdd pa;
        pa.prompt.assign(prompt, prompt + (size_t)(a_.num_codebooks + 1) * P);
        return queue_prefix(P, std::move(pa));
    }
    // a pending prefix of P positions: its pages taken, its creating pass queued (`pa` holds what the pass moves: the prompt, or an
    // imported payload).  Returns its id, or -1 when the page pool is short right now.
    int queue_prefix(int P, PendingAdd pa) {
        ensure_join_lane();
        if (!pages_.room(KvPages::kNewOwner, P).fits) return -1;
        SessPrefix px;
        px.P = P; px.live = true; px.pending = true;
        sess_prefixes_.push_back(px);
        const int owner = pages_.add_prefix();
        FS_REQUIRE(owner == pages_.prefix_owner((int)sess_prefixes_.size() - 1), "prefix ids and the page book's owners are out of step");
        pages_.grow(owner, P);
        pa.create = true; pa.L = P; pa.prefix = (int)sess_prefixes_.size() - 1; pa.owner = owner;
        sess_queue_.push_back(std::move(pa));
        return (int)sess_prefixes_.size() - 1;
    }
    SessPrefix& live_prefix(int id) {
        FS_REQUIRE(sess_active_, "no open session");
        FS_REQUIRE(id >= 0 && id < (int)sess_prefixes_.size() && sess_prefixes_[id].live, "unknown or released prefix id");
        return sess_prefixes_[id];
    }
    void session_prefix_release(int id) override {
        use_device();
        SessPrefix& px = live_prefix(id);
        px.live = false;
        if (!px.pending) pages_.drop(pages_.prefix_owner(id));  // (its pass still queued or in flight: activate_pending drops them after it)
    }
    // A prefix out of a slot's history (fishrt.h: fs_lm_session_prefix_from_slot).  The slot has T = L + n_out - 1 positions that nobody
    // writes again: a live slot's next step writes row T (it feeds its last frame there), a slot finished on its budget is parked on the
    // scratch page, and a slot frozen by <|im_end|> keeps rewriting the row its terminating iteration wrote, which is row T as well
    // (rows_frame_commit: a frozen slot neither emits nor advances).  The prefix shares the slot's first P / 64 pages and, when P is not
    // page-aligned, owns a copy of the slot's page P / 64 -- so from page T / 64 on everything stays the slot's alone.  Nothing is
    // prefilled and nothing is queued: the prefix is active when the call returns.
    int session_prefix_from_slot(int slot, int n_positions, int* P_out) override {
        use_device();
        // 1. whatever makes the request a bad one, before anything is taken or changed
        FS_REQUIRE(sess_active_, "no open session");
        FS_REQUIRE(!sess_.rows, "fs_lm_session_prefix_from_slot: FS_SESSION_ROWS sessions are not supported (their rows terminate by the row kernels' own "
                                "budget word and their launch shape depends on the highest live slot); use a plain or FS_SESSION_PER_SLOT session");
        require_live_slot(slot);
        while (slot_prefilling(slot)) { flush_pending(); activate_pending(true); }  // (its prefill is queued or in flight: let it finish first)
        const int L = sess_L_[slot], T = L + sess_hs_[slot].n_out - 1;
        if (T < 1) throw Error("T = " + std::to_string(T) + ": the slot has no history yet (a one-column prompt before its first step has no cached position)");
        if (n_positions != -1 && (n_positions < 1 || n_positions > T))
            throw Error("n_positions = " + std::to_string(n_positions) + " outside [1, T = " + std::to_string(T) + "] (-1 takes all T; T = L + n_frames - 1: the "
                        "column of the last emitted frame is not history)");
        const int P = n_positions == -1 ? T : n_positions;
        if (P >= a_.max_seq_len) throw Error("P = " + std::to_string(P) + " >= max_seq_len: the prefix leaves no room for a body within max_seq_len");
        // 2. room right now?  (reads only; the one page a cut inside a page needs)
        const int nfull = P / KV_PAGE;  // (a slot's owner in the page book is its index)
        FS_REQUIRE((int)pages_.of(slot).size() * KV_PAGE >= P, "the slot holds fewer pages than its history");
        const KvPages::Share shared{slot, nfull};
        if (!pages_.room(KvPages::kNewOwner, P, shared).fits) {
            if (P_out) *P_out = P;
            return -1;
        }
        if (P % KV_PAGE && !d_promo_pair_.p) d_promo_pair_.alloc(sizeof(int) * 2);
        // 3. the prefix: references on the slot's full pages, then its own last page (neither can fail: step 2 asked for exactly this)
        SessPrefix px;
        px.P = P; px.live = true; px.pending = false;
        sess_prefixes_.push_back(px);
        const int id = (int)sess_prefixes_.size() - 1, owner = pages_.add_prefix();
        FS_REQUIRE(owner == pages_.prefix_owner(id), "prefix ids and the page book's owners are out of step");
        pages_.share(owner, shared);
        pages_.grow(owner, P);
        if (P % KV_PAGE) {
            // the slot's page P / 64 into the prefix's own, on the decode stream: behind every step enqueued so far, and finished before
            // this returns, so ahead of whatever is queued on the prefix afterwards (and of the slot's next step, which writes that page)
            const int pair[2] = {pages_.of(slot)[(size_t)nfull], pages_.of(owner)[(size_t)nfull]};
            FS_HIP(hipMemcpyAsync(d_promo_pair_.p, pair, sizeof(pair), hipMemcpyHostToDevice, st_));
            const size_t page_bytes = page_elems_ * sizeof(KT);
            launch_kv_page_copy(kv_pool_.p, 2 * a_.n_layer, (size_t)n_pages_ * page_bytes, page_bytes, d_promo_pair_.as<int>(), 1, st_);
            FS_HIP(hipStreamSynchronize(st_));  // (pair is a local)
            sess_count_[3] += 1;
        }
        pages_.writable_from(slot, T);  // (the source's write target and everything behind it is still its alone)
        if (P_out) *P_out = P;
        return id;
    }
    // fishrt.h: fs_lm_session_last_frame -- SeqState::prev of the host mirror, which session_step refreshes after every chunk
    void session_last_frame(int slot, uint32_t* column) override {
        use_device();
        FS_REQUIRE(sess_active_, "no open session");
        require_live_slot(slot);
        FS_REQUIRE(!slot_prefilling(slot) && sess_hs_[slot].n_out > 0 && sess_hs_[slot].have_prev, "the slot has not emitted a frame yet (fs_lm_session_last_frame needs its first step)");
        for (int i = 0; i <= a_.num_codebooks; ++i) column[i] = sess_hs_[slot].prev[i];
    }
    void session_info(int64_t out[8]) override {
        int64_t live = 0;
        for (const SessPrefix& px : sess_prefixes_) live += px.live;
        out[0] = pages_.free_count(); out[1] = pages_.shared_count(); out[2] = live;
        for (int k = 0; k < 4; ++k) out[3 + k] = sess_count_[k];
        out[7] = (int64_t)std::llround(sess_pf_ms_ * 1000.0);
    }
    // ---- prefix KV blobs (fishrt.h: fs_lm_weights_fingerprint / fs_lm_session_prefix_export / _import)
    uint64_t weights_fingerprint() override {
        use_device();
        require_loaded();
        if (!fp_valid_) {
            hipStream_t s = st_pf_ ? st_pf_ : st_;  // (inside a session: not the decode stream)
            if (!d_fp_.p) d_fp_.alloc(sizeof(uint64_t));
            FS_REQUIRE(arena_bytes_ / 4 < (1ull << 32), "weight arena too large for the fingerprint's swap guarantee");
            uint64_t z = 0;
            FS_HIP(hipMemsetAsync(d_fp_.p, 0, sizeof(uint64_t), s));
            launch_arena_fingerprint(arena_.p, arena_bytes_, d_fp_.as<uint64_t>(), s);
            FS_HIP(hipMemcpyAsync(&z, d_fp_.p, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            FS_HIP(hipStreamSynchronize(s));
            z ^= (uint64_t)(arena_bytes_ / 4) * 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            fp_ = z ^ (z >> 31);
            fp_valid_ = true;
        }
        return fp_;
    }
    static constexpr uint32_t kv_dtype_id() { return std::is_same<KT, float>::value ? (uint32_t)FS_F32 : (uint32_t)FS_BF16; }
    size_t prefix_payload_bytes(int P) const { return (size_t)a_.n_layer * 2 * (size_t)P * a_.n_local_heads * a_.head_dim * sizeof(KT); }
    // grow the staging buffer / the page-id buffer (the prefill stream is drained first: an earlier pass may still read them)
    void kvb_reserve(size_t bytes, size_t n_page_ids) {
        if (d_kvb_.n >= bytes && d_kvb_pages_.n >= sizeof(int) * n_page_ids) return;
        FS_HIP(hipStreamSynchronize(st_pf_));
        if (d_kvb_.n < bytes) d_kvb_.alloc(bytes);
        if (d_kvb_pages_.n < sizeof(int) * n_page_ids) d_kvb_pages_.alloc(sizeof(int) * std::max(n_page_ids, (size_t)max_pages_));
    }
    void session_prefix_export(int id, void* blob_out, size_t cap, size_t* bytes) override {
        use_device();
        const int P = live_prefix(id).P;
        const size_t payload = prefix_payload_bytes(P), total = sizeof(fs_kv_blob_header) + payload;
        if (bytes) *bytes = total;
        if (!blob_out) return;
        FS_REQUIRE(cap >= total, "blob_out capacity is smaller than the prefix blob (query the size with blob_out == NULL)");
        while (sess_prefixes_[id].pending) { flush_pending(); activate_pending(true); }  // (its own pass first, as session_release does for a slot)
        fs_kv_blob_header h = {};
        std::memcpy(h.magic, "FSKVPFX1", 8);
        h.version = 1; h.kv_dtype = kv_dtype_id();
        h.n_layer = a_.n_layer; h.n_local_heads = a_.n_local_heads; h.head_dim = a_.head_dim; h.P = P;
        h.header_bytes = (uint32_t)sizeof(h);
        h.weights_fingerprint = weights_fingerprint();
        h.payload_bytes = payload;
        const std::vector<int>& pg = pages_.of(pages_.prefix_owner(id));
        FS_REQUIRE((int)pg.size() * KV_PAGE >= P, "the prefix holds fewer pages than its length");
        kvb_reserve(payload, pg.size());
        FS_HIP(hipMemcpyAsync(d_kvb_pages_.p, pg.data(), sizeof(int) * pg.size(), hipMemcpyHostToDevice, st_pf_));
        const size_t page_bytes = page_elems_ * sizeof(KT);
        launch_kv_rows_gather(kv_pool_.p, 2 * a_.n_layer, (size_t)n_pages_ * page_bytes, page_bytes, d_kvb_pages_.as<int>(), P, a_.n_local_heads,
                              a_.head_dim, sizeof(KT), d_kvb_.p, st_pf_);
        FS_HIP(hipMemcpyAsync(static_cast<uint8_t*>(blob_out) + sizeof(h), d_kvb_.p, payload, hipMemcpyDeviceToHost, st_pf_));
        FS_HIP(hipStreamSynchronize(st_pf_));
        std::memcpy(blob_out, &h, sizeof(h));
    }
    int session_prefix_import(const void* blob, size_t bytes) override {
        use_device();
        FS_REQUIRE(sess_active_, "no open session");
        fs_kv_blob_header h;
        FS_REQUIRE(bytes >= sizeof(h), "prefix blob: bytes is smaller than the 64-byte header");
        std::memcpy(&h, blob, sizeof(h));
        FS_REQUIRE(std::memcmp(h.magic, "FSKVPFX1", 8) == 0, "prefix blob: wrong magic (not \"FSKVPFX1\")");
        FS_REQUIRE(h.version == 1, "prefix blob: unsupported version (this library reads version 1)");
        FS_REQUIRE(h.header_bytes == sizeof(h), "prefix blob: header_bytes is not 64");
        FS_REQUIRE((uint64_t)(bytes - sizeof(h)) == h.payload_bytes, "prefix blob: bytes != 64 + payload_bytes (truncated or padded blob)");
        FS_REQUIRE(h.kv_dtype == kv_dtype_id(), "prefix blob: kv_dtype differs from this handle's KV storage type");
        FS_REQUIRE(h.n_layer == a_.n_layer, "prefix blob: n_layer differs from this handle's");
        FS_REQUIRE(h.n_local_heads == a_.n_local_heads, "prefix blob: n_local_heads differs from this handle's");
        FS_REQUIRE(h.head_dim == a_.head_dim, "prefix blob: head_dim differs from this handle's");
        FS_REQUIRE(h.P >= 1 && h.P < a_.max_seq_len, "prefix blob: P outside 1 <= P < max_seq_len (a prefix must leave room for a body)");
        FS_REQUIRE(h.payload_bytes == (uint64_t)prefix_payload_bytes(h.P), "prefix blob: payload_bytes does not match n_layer * 2 * P * n_local_heads * head_dim elements");
        FS_REQUIRE(h.weights_fingerprint == weights_fingerprint(), "prefix blob: weights_fingerprint differs from this handle's (other weights or storage type)");
        PendingAdd pa;
        pa.import_kv = true;
        const uint8_t* payload = static_cast<const uint8_t*>(blob) + sizeof(h);
        pa.blob.assign(payload, payload + h.payload_bytes);  // (the caller may free its blob as soon as this returns)
        return queue_prefix(h.P, std::move(pa));
    }
    // the pass of the imports at the head of the (sorted) queue: per import one host-to-device copy into the staging buffer and one
    // k_kv_rows_scatter into its pages, on the prefill stream; activated like a creating pass (pa.create).  No counter of a transformer
    // pass moves.
    void launch_import_pass(size_t n) {
        size_t total = 0, n_ids = 0;
        for (size_t i = 0; i < n; ++i) {  // (everything is checked before the first launch)
            const SessPrefix& px = sess_prefixes_[sess_queue_[i].prefix];
            const int owner = pages_.prefix_owner(sess_queue_[i].prefix);
            FS_REQUIRE(sess_queue_[i].blob.size() == prefix_payload_bytes(px.P) && (int)pages_.of(owner).size() * KV_PAGE >= px.P,
                       "prefix import: payload / pages do not match P");
            // (slots already queued on this prefix hold references on its pages too; none of them reads or writes one before this pass)
            FS_REQUIRE(pages_.intact(owner), "prefix import: a page of the prefix is not held");
            total += sess_queue_[i].blob.size();
            n_ids += pages_.of(owner).size();
        }
        kvb_reserve(total, n_ids);
        std::vector<int>& ids = sess_stage_imp_pages_;  // (alive until the pass has been activated)
        ids.clear();
        for (size_t i = 0; i < n; ++i) {
            const auto& pg = pages_.of(pages_.prefix_owner(sess_queue_[i].prefix));
            ids.insert(ids.end(), pg.begin(), pg.end());
        }
        FS_HIP(hipMemcpyAsync(d_kvb_pages_.p, ids.data(), sizeof(int) * ids.size(), hipMemcpyHostToDevice, st_pf_));
        const size_t page_bytes = page_elems_ * sizeof(KT);
        size_t off = 0, id_off = 0;
        for (size_t i = 0; i < n; ++i) {
            const PendingAdd& pa = sess_queue_[i];
            const SessPrefix& px = sess_prefixes_[pa.prefix];
            uint8_t* stage = d_kvb_.as<uint8_t>() + off;  // (payloads are whole 16-byte units: head_dim % 8 == 0)
            FS_HIP(hipMemcpyAsync(stage, pa.blob.data(), pa.blob.size(), hipMemcpyHostToDevice, st_pf_));
            launch_kv_rows_scatter(kv_pool_.p, 2 * a_.n_layer, (size_t)n_pages_ * page_bytes, page_bytes, d_kvb_pages_.as<int>() + id_off, px.P,
                                   a_.n_local_heads, a_.head_dim, sizeof(KT), stage, st_pf_);
            off += pa.blob.size();
            id_off += pages_.of(pages_.prefix_owner(pa.prefix)).size();
        }
    }
    // the pass of the first n queued entries is on the prefill stream: its end is marked (timing event, then the event activate_pending
    // waits for) and the entries are in flight
    void pass_launched(size_t n) {
        FS_HIP(hipEventRecord(ev_pft_[1], st_pf_));
        FS_HIP(hipEventRecord(ev_pf_, st_pf_));
        sess_flight_.assign(std::make_move_iterator(sess_queue_.begin()), std::make_move_iterator(sess_queue_.begin() + n));
        sess_queue_.erase(sess_queue_.begin(), sess_queue_.begin() + n);
    }
    // launch the prefill of the next group of queued requests (ONE pass on the prefill stream, nothing waited for); no-op while an
    // earlier group is still in flight -- the rest of the queue follows once that one has been activated.
    // Imported prefixes (fs_lm_session_prefix_import) go first, all of them in ONE pass of their own kind (launch_import_pass: copies and
    // scatters, no transformer pass): whatever was queued with them -- creations, adds, an add with a one-column body that prefills nothing --
    // stays queued until that pass has been activated.
    // Shared prefixes: a prefix's own pass (pa.create) prefills all P of its positions into its pages; creations go in passes of their
    // own, ahead of every add queued with them (an add on a prefix reads its pages, and stream order on the prefill stream puts that
    // read after the creating pass).  A prefixed member starts at position P (RowsCtx.seq_states in a group pass) and runs its body
    // columns only; when P % 64 != 0 its first private page first gets a copy of the prefix's partly filled last page (k_kv_page_copy,
    // one launch for the pass, in stream order ahead of it).
    void flush_pending() {
        if (sess_queue_.empty() || !sess_flight_.empty()) return;
        // which pass (fs_prefill_plan.h: the order of the queue, the kind of the pass, its members -- the first ps.n of the ordered queue)
        const PrefillPlan plan = plan_prefill({sess_queue_.begin(), sess_queue_.end()}, pages_, {kRowsCap, B_, a_.max_seq_len, a_.head_dim == 64});
        std::vector<PendingAdd> ordered;
        ordered.reserve(sess_queue_.size());
        for (int j : plan.order) ordered.push_back(std::move(sess_queue_[(size_t)j]));
        sess_queue_.swap(ordered);
        const PrefillPass& ps = plan.pass;
        FS_HIP(hipEventRecord(ev_pft_[0], st_pf_));
        sess_timed_ = true;
        if (ps.kind != PrefillPass::Imports) launch_tail_copies(sess_queue_.begin(), sess_queue_.begin() + ps.n);
        switch (ps.kind) {
        case PrefillPass::Imports: launch_import_pass((size_t)ps.n); break;
        case PrefillPass::NoRows: break;  // only one-column bodies are left: no pass, they go live at the next activation
        case PrefillPass::Single: join_single(sess_queue_[0]); break;
        case PrefillPass::Group: join_group(ps); break;
        }
        // (an import moves no counter of a transformer pass: it runs no row and reuses nothing)
        sess_count_[0] += ps.kind == PrefillPass::Single || ps.kind == PrefillPass::Group;
        for (int s = 0; s < ps.n; ++s) { sess_count_[1] += sess_queue_[s].rows(); sess_count_[2] += sess_queue_[s].create ? 0 : sess_queue_[s].start; }
        pass_launched((size_t)ps.n);
    }
    // one sequence on the join lane: its page list in the staging row B_, its columns staged, the staging state at its first position
    void join_single(const PendingAdd& pa) {
        if (!pa.create) pages_.writable_from(pa.slot, pa.start);
        upload_row(B_, st_pf_, pages_.of(pa.owner));
        const int cols = pa.cols();
        join_.stage_prompt(pa.prompt.data(), (size_t)(a_.num_codebooks + 1) * cols);
        sess_stage_ = SeqState{};
        sess_stage_.prompt_L = cols;
        sess_stage_.pos = pa.start;  // (a prefixed member: its body's first column sits at position P)
        FS_HIP(hipMemcpyAsync(state(B_), &sess_stage_, sizeof(SeqState), hipMemcpyHostToDevice, st_pf_));
        launch_seq_pass(join_, state(B_), B_, pa.start, pa.rows());
    }
    // the first ps.n queued members side by side on the join lane, right-padded to ps.Lp rows: page lists in the staging rows B_ .., each
    // grown to where its pad rows write (the plan has asked the book for exactly this)
    void join_group(const PrefillPass& ps) {
        const int C1 = a_.num_codebooks + 1, S = ps.n, Lp = ps.Lp;
        const size_t pstride = (size_t)C1 * Lp;
        std::vector<uint32_t>& padded = sess_stage_prompts_;  // (members: alive until the pass has been activated)
        std::vector<int>& rows = sess_stage_rows_;
        std::vector<SeqState>& pos0 = sess_stage_pos0_;
        padded.assign(pstride * S, 0u);
        rows.assign((size_t)S * max_pages_, sess_scratch_);
        pos0.assign(S, SeqState{});
        for (int s = 0; s < S; ++s) {
            const PendingAdd& pa = sess_queue_[s];
            pages_.grow(pa.owner, ps.pad_end[s]);  // (pad rows; a prefix's are trimmed at activation)
            if (!pa.create) pages_.writable_from(pa.slot, pa.start);
            const int n = pa.rows(), cols = pa.cols();
            for (int r = 0; r < C1; ++r) std::memcpy(&padded[pstride * s + (size_t)r * Lp], &pa.prompt[(size_t)r * cols], sizeof(uint32_t) * n);
            const auto& pg = pages_.of(pa.owner);
            std::copy(pg.begin(), pg.end(), rows.begin() + (size_t)s * max_pages_);
            pos0[s].pos = pa.start;
        }
        join_.stage_prompt(padded.data(), padded.size());
        upload_row(B_, st_pf_, rows);
        sess_stage_ = SeqState{};
        sess_stage_.prompt_L = Lp;
        FS_HIP(hipMemcpyAsync(state(B_), &sess_stage_, sizeof(SeqState), hipMemcpyHostToDevice, st_pf_));
        // (members that all start at 0 keep the plain group pass)
        if (ps.max_start > 0) FS_HIP(hipMemcpyAsync(d2_seqpos_.p, pos0.data(), sizeof(SeqState) * S, hipMemcpyHostToDevice, st_pf_));
        launch_group_pass(join_, join_.prompt.as<uint32_t>(), S, Lp, pstride, state(B_), B_, ps.max_start > 0 ? d2_seqpos_.as<SeqState>() : nullptr,
                          chunk_bucket(ps.max_start + Lp));
    }
    // copy-on-write of the partly filled last page of a prefix into the joining slot's first private page, for all members of a pass
    // that need it: ONE k_kv_page_copy launch over every slow layer's K and V pools, on the prefill stream ahead of the pass
    template <typename It>
    void launch_tail_copies(It first, It last) {
        std::vector<int>& pairs = sess_stage_copy_;  // (alive until the pass has been activated)
        pairs.clear();
        for (It it = first; it != last; ++it)
            if (!it->create && it->tail >= 0) {
                pages_.writable_from(it->slot, it->start);
                pairs.push_back(it->tail);
                pairs.push_back(pages_.of(it->slot)[it->start / KV_PAGE]);
            }
        if (pairs.empty()) return;
        const int n = (int)pairs.size() / 2;
        FS_REQUIRE(n <= B_, "more tail copies than slots");
        FS_HIP(hipMemcpyAsync(d2_copy_.p, pairs.data(), sizeof(int) * pairs.size(), hipMemcpyHostToDevice, st_pf_));
        const size_t page_bytes = page_elems_ * sizeof(KT);
        launch_kv_page_copy(kv_pool_.p, 2 * a_.n_layer, (size_t)n_pages_ * page_bytes, page_bytes, d2_copy_.as<int>(), n, st_pf_);
        sess_count_[3] += n;
    }
    // the requests whose prefill is in flight (if it has finished, or after waiting for it) become live slots; called between steps only
    void activate_pending(bool wait) {
        if (sess_flight_.empty()) return;
        if (!wait) {
            const hipError_t q = hipEventQuery(ev_pf_);
            if (q == hipErrorNotReady) return;
            FS_HIP(q);
        }
        FS_HIP(hipEventSynchronize(ev_pf_));
        if (sess_timed_) {
            float ms = 0.f;
            FS_HIP(hipEventElapsedTime(&ms, ev_pft_[0], ev_pft_[1]));
            sess_pf_ms_ += ms;
            sess_timed_ = false;
        }
        const int C1 = a_.num_codebooks + 1;
        // per-slot sampler streams of the joining slots, staged here until the stream has been waited for below
        std::vector<SlotRng> up_rng;
        up_rng.reserve(sess_flight_.size());
        std::vector<ScoreSlot> up_tr;  // ... and the device table entries of the traced ones
        up_tr.reserve(sess_flight_.size());
        for (const PendingAdd& pa : sess_flight_) {
            if (pa.create) {  // the prefix's K/V are in place: its pad pages go back; a prefix released meanwhile goes now
                SessPrefix& px = sess_prefixes_[pa.prefix];
                px.pending = false;
                pages_.truncate(pages_.prefix_owner(pa.prefix), px.P);
                if (!px.live) pages_.drop(pages_.prefix_owner(pa.prefix));
                continue;
            }
            if (pa.tail >= 0) pages_.drop_hold(pa.tail);  // (copied: the joining slot's hold on the prefix's last page ends)
            const int b = pa.slot, L = pa.L, Lp = L - 1, cols = pa.cols();
            pages_.writable_from(b, Lp);
            upload_row(b, st_, pages_.of(b));
            seq_len_[b] = Lp;
            SeqState ss = {};
            ss.pos = Lp; ss.prompt_L = L; ss.step = Lp;
            for (int r = 0; r < C1; ++r) ss.cur[r] = pa.prompt[(size_t)r * cols + (cols - 1)];
            sess_hs_[b] = ss;
            FS_HIP(hipMemcpyAsync(state(b), &sess_hs_[b], sizeof(SeqState), hipMemcpyHostToDevice, st_));
            // the slot's own settings / seed (fs_lm_session_add_ex), or the session's back after an occupant that had its own.  (The copies
            // read pa / sess_cfg_, which outlive the wait below.)
            const SampleCfg& cfg = pa.has_cfg ? pa.cfg : sess_cfg_;
            const uint64_t seed = pa.has_seed ? pa.seed : sess_seed_ + (uint64_t)pa.order;
            if (sess_.rows) {  // the slot becomes a live row: first-frame input, iteration budget, fresh repetition-penalty window and sampler stream
                LmKernels<WT>::embed(d_, tok_emb_, cb_emb_, a_.num_codebooks, a_.codebook_size, d_cfg_.as<SampleCfg>(), nullptr, state(b), x(b), st_);
                sess_budget_tmp_ = pa.n_iter;
                FS_HIP(hipMemcpyAsync(d_rbudget_.as<int>() + b, &sess_budget_tmp_, sizeof(int), hipMemcpyHostToDevice, st_));
                RngState rng;
                upload_rng(seed, rng, d_rrng_.as<RngState>() + b, st_);
                FS_HIP(hipMemcpyAsync(d_rcfg_.as<SampleCfg>() + b, &cfg, sizeof(SampleCfg), hipMemcpyHostToDevice, st_));
                launch_reppen_reset(rrp_.view(b), a_.num_codebooks, a_.codebook_size, st_);
                FS_HIP(hipStreamSynchronize(st_));  // (rng / budget are locals)
            } else {
                if (sess_.slots) {  // the slot's settings, a StdRng stream at word 0 (no look-ahead word yet) and empty repetition-penalty windows
                    up_rng.push_back(slot_rng_fresh(seed));
                    FS_HIP(hipMemcpyAsync(d_scfg_.as<SampleCfg>() + b, &cfg, sizeof(SampleCfg), hipMemcpyHostToDevice, st_));
                    FS_HIP(hipMemcpyAsync(d_srng_.as<SlotRng>() + b, &up_rng.back(), sizeof(SlotRng), hipMemcpyHostToDevice, st_));
                    launch_reppen_reset(srp_.view(b), a_.num_codebooks, a_.codebook_size, st_);
                }
                LmKernels<WT>::embed(d_, tok_emb_, cb_emb_, a_.num_codebooks, a_.codebook_size, d_cfg_.as<SampleCfg>(), nullptr, state(b),
                                     main_.x.as<float>() + (size_t)b * a_.dim, st_);
            }
            if (pa.hid.p) tab_activate(hid_, b, pa.hid);  // (its first iteration is the step that runs its last prompt position)
            if (pa.sc.p && pa.traced) {  // a traced slot: the device entry is a scoring slot's WITHOUT targets (the book's own keeps the pointer:
                // the token rows live there).  No row of the stash is open between two steps: the tail node closes what a step opened.
                up_tr.push_back(sc_.book.activate(b, pa.sc));
                up_tr.back().targets = nullptr;
                FS_HIP(hipMemcpyAsync(sc_.dev.as<ScoreSlot>() + b, &up_tr.back(), sizeof(ScoreSlot), hipMemcpyHostToDevice, st_));
            } else if (pa.sc.p) {  // the targets into the slot's buffer first
                FS_REQUIRE(pa.n_iter <= pa.sc.cap && pa.sc_targets.size() == (size_t)pa.n_iter * C1, "score buffer shorter than the slot's iterations");
                FS_HIP(hipMemcpyAsync(score_targets(pa.sc), pa.sc_targets.data(), sizeof(uint32_t) * pa.sc_targets.size(), hipMemcpyHostToDevice, st_));
                tab_activate(sc_, b, pa.sc);
            }
            sess_left_[b] = pa.n_iter;
            sess_pos_[b] = Lp;
            sess_L_[b] = L;
        }
        FS_HIP(hipStreamSynchronize(st_));
        sess_flight_.clear();
    }
    void ensure_join_lane() {
        if (join_.x.p) return;
        FS_HIP(hipStreamCreateWithFlags(&st_pf_, hipStreamNonBlocking));
        FS_HIP(hipEventCreateWithFlags(&ev_pf_, hipEventDisableTiming));
        for (hipEvent_t& e : ev_pft_) FS_HIP(hipEventCreate(&e));  // (timed: fs_lm_session_info's prefill-stream time)
        d2_seqpos_.alloc(sizeof(SeqState) * (size_t)B_);
        d2_copy_.alloc(sizeof(int) * 2 * (size_t)B_);
        join_.ensure(a_, down_split_, n_chunks_, d_cos_.as<float>(), d_sin_.as<float>());  // (down_split_: the main lane's, ensured at session begin)
        FS_HIP(hipStreamSynchronize(st_pf_));
    }
    void session_step(int n_frames, int* n_active) override {
        use_device();
        FS_REQUIRE(sess_active_, "no open session");
        FS_HIP(hipEventRecord(ev_[1], st_));
        int launched = 0;
        while (launched < n_frames) {
            flush_pending();                   // queued requests start their (group) prefill on the second stream
            activate_pending(/*wait=*/false);  // a finished prefill joins here, between two replays of the step graph
            int chunk = n_frames - launched, longest = 0, live = 0;
            for (int b = 0; b < B_; ++b)
                if (slot_running(b)) { chunk = std::min(chunk, sess_left_[b]); longest = std::max(longest, sess_pos_[b]); ++live; }
            if (!live && (!sess_flight_.empty() || !sess_queue_.empty())) {
                // nothing else to run (a burst into an idle session): admit everything queued, group pass after group pass, then step
                while (!sess_flight_.empty() || !sess_queue_.empty()) { flush_pending(); activate_pending(true); }
                continue;
            }
            if (!live) break;
            if (sess_.rows) {
                PersistFlagsGuard flags_guard{*this};
                use_persist_ = true; use_pslow_ = true; persist_sampled_ = sess_.sampled;
                // the launch group covers slots [0, top): the smallest instantiations that hold the highest live slot (an 8-slot session with two
                // live requests in slots 0, 1 pays the 2-row frame, 0.84 ms, not the 8-row one, 1.67 ms); slots are handed out lowest-first
                int top = 0;
                for (int b = 0; b < B_; ++b)
                    if (slot_running(b)) top = b + 1;
                const int Rs = std::min(sess_.R, top <= 2 ? 2 : (top <= 4 ? 4 : 8));
                for (int i = 0; i < chunk; ++i) {
                    set_bucket(longest + i + 1);
                    launch_rows_slow(rows_slow_args(Rs), Rs, st_);
                    // (x(r) now holds row r's pre-norm hidden state; the fast launches overwrite it with the next input)
                    if (hid_.book.live() > 0) launch_hidden_rows(hid_.dev.as<HidSlot>(), state(0), x(0), a_.dim, top, st_);
                    launch_rows_fast_groups(top, sess_.sampled);
                }
            } else
            for (int i = 0; i < chunk; ++i) {
                set_bucket(longest + i + 1);
                FS_HIP(hipGraphLaunch(batch_graph(B_), st_));
            }
            launched += chunk;
            for (int b = 0; b < B_; ++b)
                if (slot_running(b)) {
                    sess_left_[b] -= chunk; sess_pos_[b] += chunk;
                    if (sess_left_[b] == 0 && !sess_.rows) {  // iteration budget spent: the slot is finished whatever it sampled (rows mode: the kernels' own budget word terminates the row)
                        // Its last iteration left pos = L + n_iter - 1, one token PAST its page allocation (and == max_seq_len when the
                        // budget was clamped), and a frozen slot still rides the step graphs, whose QKV epilogue writes K/V at pos: park
                        // the write on the scratch page at position 0 (n_out and the codes stay) before the next replay can run.
                        static const int one = 1, zero = 0;
                        FS_HIP(hipMemcpyAsync(&state(b)->done, &one, sizeof(int), hipMemcpyHostToDevice, st_));
                        FS_HIP(hipMemcpyAsync(&state(b)->pos, &zero, sizeof(int), hipMemcpyHostToDevice, st_));
                        upload_row(b, st_, &sess_scratch_, 1);
                    }
                }
            // (a slot that sampled <|im_end|> inside the chunk froze itself on the device; the host learns it below)
            FS_HIP(hipMemcpyAsync(sess_hs_.data(), state(0), sizeof(SeqState) * B_, hipMemcpyDeviceToHost, st_));
            tab_fetch_counts(hid_);  // (the row counts)
            tab_fetch_counts(sc_);   // (the record counts)
            FS_HIP(hipStreamSynchronize(st_));
            tab_take_counts(hid_);
            tab_take_counts(sc_);
            // a spin timeout inside the chunk (the joining prefill shares the CUs the persistent launches need co-resident) means the slots'
            // codes are garbage: raise instead of handing them out; the caller ends the session (the handle is off the row path afterwards)
            if (sess_.rows) rows_check_ctl(/*include_b1_fast=*/false);
            else check_rows_xchg();
        }
        FS_HIP(hipEventRecord(ev_[2], st_));
        FS_HIP(hipEventSynchronize(ev_[2]));
        float ms = 0;
        FS_HIP(hipEventElapsedTime(&ms, ev_[1], ev_[2]));
        stats_.decode_ms += ms;
        stats_.graph_launches += (uint64_t)launched;
        int act = 0;
        uint64_t frames = 0;
        for (int b = 0; b < B_; ++b) {
            if (slot_running(b) || slot_prefilling(b)) ++act;
            if (sess_left_[b] >= 0) frames += (uint64_t)sess_hs_[b].n_out;
        }
        stats_.frames = sess_released_frames_ + frames;
        if (n_active) *n_active = act;
    }
    void session_poll(int slot, uint32_t* codes_out, size_t cap, size_t* n_frames, int* done) override {
        use_device();
        require_live_slot(slot);
        const int C = a_.num_codebooks;
        const size_t nb = slot_prefilling(slot) ? 0 : (size_t)sess_hs_[slot].n_out;
        if (codes_out) {
            FS_REQUIRE(nb <= cap, "codes_out capacity too small for the generated frames");
            for (int c = 0; c < C; ++c)
                FS_HIP(hipMemcpyAsync(codes_out + (size_t)c * cap, d_out_.as<uint32_t>() + ((size_t)slot * C + c) * out_cap_, sizeof(uint32_t) * nb,
                                      hipMemcpyDeviceToHost, st_));
            FS_HIP(hipStreamSynchronize(st_));
        }
        if (n_frames) *n_frames = nb;
        if (done) *done = (!slot_prefilling(slot) && (sess_hs_[slot].done != 0 || sess_left_[slot] == 0)) ? 1 : 0;
    }
    void session_release(int slot) override {
        use_device();
        require_live_slot(slot);
        while (slot_prefilling(slot)) { flush_pending(); activate_pending(true); }  // (its prefill is queued or in flight: let it finish first)
        sess_released_frames_ += (uint64_t)sess_hs_[slot].n_out;
        truncate(slot, 0);
        park_slot(slot, sess_.rows);
        tab_drop(hid_, slot);
        tab_drop(sc_, slot);
        sess_traced_[slot] = 0;
        sess_left_[slot] = kSlotFree;
    }
    void session_end() override {
        if (!sess_active_) return;
        use_device();
        if (!sess_flight_.empty()) (void)hipEventSynchronize(ev_pf_);
        // the page book's verdict on the session, asked once, while every owner and hold is still in place; it is raised below, when the
        // session has been closed all the same
        std::string bad_book;
        try { pages_.check(); } catch (const std::exception& e) { bad_book = e.what(); }
        // the holds of the adds still pending go first, in flight and queue order (the order pages return in decides who gets which next)
        for (auto* q : {&sess_flight_, &sess_queue_})
            for (const PendingAdd& pa : *q) if (pa.tail >= 0) pages_.drop_hold(pa.tail);
        tab_end(hid_);  // (the collector buffers of those adds were in hand: the books take them back)
        tab_end(sc_);
        sess_flight_.clear(); sess_queue_.clear();
        pages_.end_session();  // (the slots' pages, the prefixes' -- live or not: the session's references end with it -- and the scratch page)
        std::fill(seq_len_.begin(), seq_len_.end(), 0);
        sess_prefixes_.clear();
        SampleCfg cfg = base_cfg();
        FS_HIP(hipMemcpyAsync(d_cfg_.p, &cfg, sizeof(cfg), hipMemcpyHostToDevice, st_));
        FS_HIP(hipStreamSynchronize(st_));
        sess_active_ = false;
        const bool rows = sess_.rows;
        sess_ = {};
        sess_released_frames_ = 0;
        if (rows) check_ctl({&d_rctl_s_, &d_rctl_f_}, nullptr, nullptr);  // (a session that ended on an error: reset only)
        if (sess_plock_.owns_lock()) sess_plock_.unlock();
        if (!bad_book.empty()) throw Error(bad_book);
    }

    void generate_batch_sequential(const uint32_t* prompts, const int* lens, int n, int max_new_tokens, const fs_sampling& s, uint64_t seed,
                                   uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames, uint8_t* is_audio) {
        if (legacy_) throw Error("generate_static_batch samples the slow token over the full vocabulary for Fish <= 1.4 (static_batch.rs:132-141); not implemented");
        const int C1 = a_.num_codebooks + 1;
        int Lmax = 0;
        for (int i = 0; i < n; ++i) { FS_REQUIRE(lens[i] >= 1, "empty prompt"); Lmax = std::max(Lmax, lens[i]); }
        fs_sampling sb = s;
        sb.repetition_penalty = 1.0f;
        size_t off = 0;
        std::vector<uint32_t> padded((size_t)C1 * Lmax);
        for (int i = 0; i < n; ++i) {
            left_pad(prompts + off, lens[i], Lmax, padded.data());
            off += (size_t)C1 * lens[i];
            clear_slow();  // static_batch.rs:118-121
            // BatchedLogitsProcessor semantics on the single-sequence kernels (sampling/mod.rs:77-109): temp <= 1e-7 -> device argmax
            // (FIRST maximal index), else the child StdRng of (sample() call, row i) seeded from the master's u64 number call * n + i --
            // row i generated on its own draws exactly what it draws in lock-step
            batch_rows_ = n; batch_row_ = i;
            try {
                generate(padded.data(), Lmax, max_new_tokens, sb, seed, flags, codes_out + (size_t)i * a_.num_codebooks * cap, cap, &n_frames[i],
                         nullptr, nullptr, nullptr, 0, nullptr);
            } catch (...) { batch_rows_ = 0; batch_row_ = 0; throw; }
            batch_rows_ = 0; batch_row_ = 0;
            if (is_audio) {  // (one iteration executed and its slow token was <|im_end|>: the unconditional first position is not audio)
                const SeqState* hs = reinterpret_cast<const SeqState*>(h_pin_);
                const bool first_not_audio = hs->frame == 1 && hs->cur[0] == t_.im_end_id;
                for (size_t f = 0; f < n_frames[i]; ++f) is_audio[(size_t)i * cap + f] = (f == 0 && first_not_audio) ? 0 : 1;
            }
        }
    }


    // ---- R concurrent batch-1 requests on ONE device (lm_persist_rows.hip; no reference counterpart beyond the lock-step static batch,
    // generate/static_batch.rs:117-274).  Row i is generate_blocking(prompt_i, max_new_tokens_i, sampling_i) on its own KV slot, sampler,
    // repetition-penalty state and RNG stream (single_batch.rs:76-214) -- the same tokens as its own fs_lm_generate call on a cleared
    // cache (other summation order inside the kernels: greedy tokens can differ at near-ties only); every decode frame runs the slow
    // transformer of all rows as ONE persistent launch (weights streamed once for all rows) and the fast decoder as one launch per
    // group of <= 4 rows.  Handles that cannot take that path (f32 / fp8, Fish <= 1.4, sampler settings outside the in-launch sampler,
    // another call holding the device's persistent kernels) run the requests one after the other.
    void generate_multi(const uint32_t* prompts, const int* lens, int n, const int* max_new_tokens, const fs_sampling* samplings,
                        const uint64_t* seeds, uint32_t flags, uint32_t* codes_out, size_t cap, size_t* n_frames) override {
        use_device();
        require_loaded();
        FS_REQUIRE(!sess_active_, "the handle is in session mode (fs_lm_session_end first)");
        FS_REQUIRE(n >= 1, "Must have at least one prompt");
        const int C = a_.num_codebooks, C1 = C + 1;
        std::vector<size_t> poff(n);
        {
            size_t off = 0;
            for (int i = 0; i < n; ++i) { FS_REQUIRE(lens[i] >= 1, "empty prompt"); FS_REQUIRE(max_new_tokens[i] >= 0, "negative max_new_tokens"); poff[i] = off; off += (size_t)C1 * lens[i]; }
        }
        bool rows_ok = rows_supported(n, samplings) && !(flags & FS_GEN_NO_PERSIST);
        const bool rows_sampled = samplings[0].temp != 0.0;
        std::unique_lock<PersistLock> plock;
        if (rows_ok) { plock = acquire_persist(device_); rows_ok = plock.owns_lock(); }
        if (!rows_ok) {
            if (plock.owns_lock()) plock.unlock();
            double pf = 0, dc = 0; uint64_t fr = 0, pt = 0, gl = 0;
            for (int i = 0; i < n; ++i) {
                clear_slow();
                generate(prompts + poff[i], lens[i], max_new_tokens[i], samplings[i], seeds[i], flags, codes_out + (size_t)i * C * cap, cap, &n_frames[i],
                         nullptr, nullptr, nullptr, 0, nullptr);
                pf += stats_.prefill_ms; dc += stats_.decode_ms; fr += stats_.frames; pt += stats_.prompt_tokens; gl += stats_.graph_launches;
            }
            stats_.prefill_ms = pf; stats_.decode_ms = dc; stats_.frames = fr; stats_.prompt_tokens = pt; stats_.graph_launches = gl;
            return;
        }
        const int R = n <= 2 ? 2 : (n <= 4 ? 4 : 8);
        ensure_rows(R);
        clear_slow();
        clear_fast();
        std::vector<long long> n_iter(n);
        long long max_iter = 0;
        for (int i = 0; i < n; ++i) {
            validate_tokens(prompts + poff[i], 0, 1, lens[i]);
            if (lens[i] > a_.max_seq_len) throw Error("prompt exceeds max_seq_len (dual_ar.rs:623-624)");
            n_iter[i] = iter_budget(max_new_tokens[i], lens[i]).n_iter;  // (a row stops at max_seq_len)
            max_iter = std::max(max_iter, n_iter[i]);
            ensure_capacity(i, lens[i] + (int)n_iter[i] - 1);
        }
        // per-row device state: sampling configuration, iteration budget, generator state (rows >= n: terminated)
        std::vector<SampleCfg> cfgs(R);
        std::vector<int> budget(R, 0);
        for (int i = 0; i < R; ++i) {
            cfgs[i] = i < n ? make_cfg(samplings[i], flags) : base_cfg();
            if (i < n) budget[i] = (int)n_iter[i];
        }
        FS_HIP(hipMemcpyAsync(d_rcfg_.p, cfgs.data(), sizeof(SampleCfg) * R, hipMemcpyHostToDevice, st_));
        FS_HIP(hipMemcpyAsync(d_rbudget_.p, budget.data(), sizeof(int) * R, hipMemcpyHostToDevice, st_));
        float* nullp = nullptr;
        FS_HIP(hipMemcpyAsync(d_hid_slot_.p, &nullp, sizeof(nullp), hipMemcpyHostToDevice, st_));
        ensure_rows_capture(R);
        PersistFlagsGuard flags_guard{*this};
        stats_ = {};
        FS_HIP(hipEventRecord(ev_[0], st_));
        for (int i = 0; i < R; ++i) {
            SeqState ss = {};
            if (i >= n) { ss.done = 2; FS_HIP(hipMemcpyAsync(state(i), &ss, sizeof(ss), hipMemcpyHostToDevice, st_)); continue; }
            const int L = lens[i];
            ss.prompt_L = L;
            FS_HIP(hipMemcpyAsync(state(i), &ss, sizeof(ss), hipMemcpyHostToDevice, st_));
            FS_HIP(hipMemcpyAsync(main_.prompt.p, prompts + poff[i], sizeof(uint32_t) * C1 * L, hipMemcpyHostToDevice, st_));
            FS_HIP(hipMemcpyAsync(d_cfg_.p, &cfgs[i], sizeof(SampleCfg), hipMemcpyHostToDevice, st_));  // (embed reads the semantic range from d_cfg_)
            RngState rng;
            upload_rng(seeds[i], rng, d_rrng_.as<RngState>() + i, st_);
            launch_reppen_reset(rrp_.view(i), C, a_.codebook_size, st_);
            prefill_tokens(i, L - 1, /*use_graph=*/false);
            LmKernels<WT>::embed(d_, tok_emb_, cb_emb_, C, a_.codebook_size, d_cfg_.as<SampleCfg>(), main_.prompt.as<uint32_t>(), state(i), x(i), st_);
            FS_HIP(hipStreamSynchronize(st_));  // main_.prompt / d_cfg_ are reused by the next row
            seq_len_[i] = L - 1;
            stats_.prompt_tokens += (uint64_t)L;
        }
        use_persist_ = true; use_pslow_ = true; persist_sampled_ = rows_sampled;
        std::vector<SeqState> hs(R);
        auto all_done = [&]() {
            FS_HIP(hipMemcpyAsync(hs.data(), state(0), sizeof(SeqState) * R, hipMemcpyDeviceToHost, st_));
            FS_HIP(hipStreamSynchronize(st_));
            for (int i = 0; i < n; ++i) if (hs[i].done != 2) return false;
            return true;
        };
        int maxL = 0;
        for (int i = 0; i < n; ++i) maxL = std::max(maxL, lens[i]);
        const bool rows_fast = !getenv("FISHRT_ROWS_FAST_SINGLE");
        auto launch_frame = [&](long long it_) {
            set_bucket(maxL + (int)it_);
            RowsSlowArgs S = rows_slow_args(R);
            launch_rows_slow(S, R, st_);
            if (rows_fast) launch_rows_fast_groups(n, rows_sampled);
            else {
                static const int two = 2;
                for (int i = 0; i < n; ++i) {
                    if (it_ >= n_iter[i]) { if (it_ == n_iter[i]) FS_HIP(hipMemcpyAsync(&state(i)->done, &two, sizeof(int), hipMemcpyHostToDevice, st_)); continue; }
                    launch_fast_persist(persist_args(i), rows_sampled, st_);
                }
            }
        };
        launch_frame(0);
        FS_HIP(hipEventRecord(ev_[1], st_));
        long long it = 1;
        // (direct launches: 8 frames of these launches in ONE graph were measured at 940.9 vs 937.6 us per 4-row frame, 1575.5 vs 1576.7 at R = 8 --
        // back-to-back launches on a stream already pay what a graph edge does; the 7 us the batch-1 loop saved belong to hipGraphLaunch)
        while (it < max_iter) {
            const long long end = std::min<long long>(max_iter, it + 32);
            for (; it < end; ++it) launch_frame(it);
            if (it < max_iter && all_done()) break;
        }
        if (!rows_fast) {  // rows whose budget ended exactly at max_iter still need their flag
            static const int two = 2;
            for (int i = 0; i < n; ++i) FS_HIP(hipMemcpyAsync(&state(i)->done, &two, sizeof(int), hipMemcpyHostToDevice, st_));
        }
        FS_HIP(hipEventRecord(ev_[2], st_));
        FS_HIP(hipMemcpyAsync(hs.data(), state(0), sizeof(SeqState) * R, hipMemcpyDeviceToHost, st_));
        FS_HIP(hipStreamSynchronize(st_));
        use_persist_ = use_pslow_ = false;
        float ms01 = 0, ms12 = 0;
        FS_HIP(hipEventElapsedTime(&ms01, ev_[0], ev_[1]));
        FS_HIP(hipEventElapsedTime(&ms12, ev_[1], ev_[2]));
        stats_.prefill_ms = ms01; stats_.decode_ms = ms12; stats_.graph_launches = (uint64_t)it;
        stats_.kernels_per_frame = (uint64_t)(1 + (rows_fast ? (n + PR_FAST_ROWS - 1) / PR_FAST_ROWS : n));
        dump_rows_prof(R, it);
        rows_check_ctl(/*include_b1_fast=*/!rows_fast);
        stats_.frames = copy_out_rows(hs, n, codes_out, cap, n_frames);
    }

    // fs_lm_rows_supported: would fs_lm_generate_multi serve these n requests on the request-row kernels (one persistent launch group per
    // frame) rather than one after the other?  Says nothing about whether another call holds the device's persistent kernels right now.
    // ONE predicate for "these requests run on the request-row kernels" (the capability query, fs_lm_generate_multi and
    // fs_lm_session_begin(FS_SESSION_ROWS) used to carry three hand-written copies that had drifted apart).  ns = 1: one sampler setting for
    // all n rows (sessions); ns = n: one per request.  for_session: a row session's slots additionally need the Fish 1.5 token layout (the
    // legacy 2-way slow draw is per-call state of generate_multi, not of a slot) and exactly 2, 4 or 8 slots.  why (nullable): what failed.
    bool rows_predicate(int n, const fs_sampling* ss, int ns, bool for_session, const char** why = nullptr) const {
        const char* w = nullptr;
        if (!(n >= 2 && n <= PR_MAX_ROWS && n <= B_)) w = "2 <= requests <= min(8, max_batch)";
        else if (!(loaded_ && pslow_ok_ && persist_ok_ && n_audio_ <= 2048)) w = "a loaded bf16 / fp8 handle with the Fish geometry on a 256-CU device";
        else if (getenv("FISHRT_NO_ROWS")) w = "FISHRT_NO_ROWS is set";
        else if (!rows_kv_span_ok(n <= 2 ? 2 : (n <= 4 ? 4 : 8))) w = "max_seq_len too long for the row kernels' attention slices at this row count";
        else if (for_session && legacy_) w = "row SESSIONS need the Fish 1.5 token layout (fs_lm_generate_multi serves Fish <= 1.4 handles)";
        else if (for_session && !(n == 2 || n == 4 || n == 8)) w = "row sessions need max_batch 2, 4 or 8";
        else {
            // one instantiation per launch: every request greedy, or every request within the in-launch sampler (temp > 0, 0 < top_k <= 256)
            const bool sampled = ss[0].temp != 0.0;
            for (int i = 0; i < ns && !w; ++i) {
                if ((ss[i].temp != 0.0) != sampled) w = "every request greedy or every request sampled";
                else if (sampled && !fast_persist_samples((float)ss[i].temp, clamp_top_k(ss[i].top_k), a_.codebook_size)) w = "sampled requests with 0 < top_k <= 256";
            }
        }
        if (why) *why = w;
        return w == nullptr;
    }
    bool rows_supported(int n, const fs_sampling* samplings) override { return rows_predicate(n, samplings, n, /*for_session=*/false); }

  private:
    void use_device() { FS_HIP(hipSetDevice(device_)); }

    // k_slow_rows stages the page ids of ONE attention slice in 160 LDS slots (lm_persist_rows.hip `s_pages`): a slice is at most
    // ceil(max_seq_len / (16 / R)) tokens (fewer slices only while the cache is shorter than that many 128-token chunks)
    bool rows_kv_span_ok(int R) const {
        const int nslm = std::max(1, 16 / std::max(1, R));
        return ((a_.max_seq_len + nslm - 1) / nslm) / KV_PAGE + 2 <= 160;
    }
    // The persistent kernels' control words: [1] = a grid-wide wait hit its spin bound, [2] = launched with a sampler configuration the
    // instantiation was not built for (the fast decoders only).  Either way the codes of this call are garbage: read the words of every
    // buffer given and reset the ones that are set; then, unless `who` is null (session_end: reset only), raise -- after a timeout the
    // handle stays on the per-node graphs from now on, so only this request is lost.
    void check_ctl(std::initializer_list<DevBuf*> bufs, const char* who, const char* bad_cfg_msg) {
        bool timeout = false, bad_cfg = false;
        for (DevBuf* cb : bufs) {
            if (!cb || !cb->p) continue;
            uint32_t ctl[4] = {0, 0, 0, 0};
            FS_HIP(hipMemcpy(ctl, cb->p, sizeof(ctl), hipMemcpyDeviceToHost));
            if (ctl[1] || ctl[2]) FS_HIP(hipMemset((uint32_t*)cb->p + 1, 0, 8));
            timeout |= ctl[1] != 0; bad_cfg |= ctl[2] != 0;
        }
        if (!who) return;
        if (timeout) {
            pslow_ok_ = persist_ok_ = false;
            throw Error(std::string(who) + ": a grid-wide wait timed out (are all 256 CUs available to this process?); "
                                           "the handle falls back to per-node launches for its next calls");
        }
        if (bad_cfg) throw Error(bad_cfg_msg);
    }
    void rows_check_ctl(bool include_b1_fast) {
        check_ctl({&d_rctl_s_, &d_rctl_f_, include_b1_fast ? &d_ctl_ : (DevBuf*)nullptr}, "request-row persistent kernels",
                  "request-row persistent kernels launched with a sampling configuration they were not built for");
    }
    // FISHRT_PERSIST_PROF: the stage timers workgroup 0 (FISHRT_PERSIST_PROF_WG for the slow kernel) of the batch-1 persistent kernels
    // accumulated over this call, read and reset
    void dump_persist_prof(int L) {
        if (!getenv("FISHRT_PERSIST_PROF")) return;
        unsigned long long pr[24];
        const double f = 0.01 / std::max<double>(1.0, (double)stats_.graph_launches - (double)L + 1);  // us per frame
        if (use_persist_) {
            FS_HIP(hipMemcpy(pr, d_ctl_.as<uint32_t>() + 16, sizeof(pr), hipMemcpyDeviceToHost));
            FS_HIP(hipMemset(d_ctl_.as<uint32_t>() + 16, 0, sizeof(pr)));
            fprintf(stderr, "persist prof (us/frame, workgroup 0; wait+work): preload %.1f  S1 %.1f+%.1f  S2 %.1f+%.1f  S3 %.1f+%.1f  S4 %.1f+%.1f  head %.1f+%.1f  decision %.1f+%.1f  tail %.1f | S3 split: gemv+reduce %.1f barrier %.1f epilogue %.1f\n",
                    pr[0] * f, pr[9] * f, pr[1] * f, pr[10] * f, pr[2] * f, pr[11] * f, pr[3] * f, pr[12] * f, pr[4] * f, pr[13] * f, pr[5] * f, pr[14] * f, pr[6] * f, pr[7] * f, pr[8] * f, pr[15] * f, pr[3] * f);
            fprintf(stderr, "persist boundaries (us/frame, workgroup 0): slow kernel's finish -> fast kernel's entry %.2f (%llu frames)  entry -> first stage timer (state, slow-token decision) %.2f  last timer -> finish %.2f\n",
                    pr[20] ? pr[17] * 0.01 / (double)pr[20] : 0.0, pr[20], pr[18] * f, pr[19] * f);
        }
        if (use_pslow_) {
            FS_HIP(hipMemcpy(pr, d_sctl_.as<uint32_t>() + 16, sizeof(pr), hipMemcpyDeviceToHost));
            FS_HIP(hipMemset(d_sctl_.as<uint32_t>() + 16, 0, sizeof(pr)));
            fprintf(stderr, "slow persist prof (us/frame, workgroup %d; wait+work): S1 %.1f+%.1f  S2 %.1f+%.1f  S3 %.1f+%.1f  S4 %.1f+%.1f  S5 %.1f+%.1f  head %.1f+%.1f\n",
                    getenv("FISHRT_PERSIST_PROF_WG") ? atoi(getenv("FISHRT_PERSIST_PROF_WG")) : 0, pr[9] * f, pr[1] * f, pr[10] * f, pr[2] * f, pr[11] * f, pr[3] * f,
                    pr[12] * f, pr[4] * f, pr[13] * f, pr[5] * f, pr[14] * f, pr[6] * f);
            fprintf(stderr, "slow persist boundaries (us/frame): fast kernel's finish -> slow kernel's entry %.2f (%llu frames)  entry -> first stage timer (state, first loads) %.2f  last timer -> finish %.2f\n",
                    pr[20] ? pr[17] * 0.01 / (double)pr[20] : 0.0, pr[20], pr[18] * f, pr[19] * f);
        }
    }
    void dump_rows_prof(int R, long long frames) {  // the same for the request-row kernels
        if (!getenv("FISHRT_PERSIST_PROF")) return;
        unsigned long long pr[16];
        const double f = 0.01 / std::max<double>(1.0, (double)frames);  // us per frame (wall_clock64 ticks are 10 ns)
        FS_HIP(hipMemcpy(pr, d_rctl_s_.as<uint32_t>() + 16, sizeof(pr), hipMemcpyDeviceToHost));
        FS_HIP(hipMemset(d_rctl_s_.as<uint32_t>() + 16, 0, sizeof(pr)));
        fprintf(stderr, "rows slow prof R=%d (us/frame, workgroup 0): S1 %.1f  S2 %.1f  S3 sweep %.1f + %.1f  S4 sweep %.1f gemm %.1f barrier %.1f publish %.1f  S5 sweep+gemm %.1f barrier %.1f publish %.1f  head %.1f\n",
                R, pr[1] * f, pr[2] * f, pr[8] * f, pr[3] * f, pr[9] * f, pr[10] * f, pr[11] * f, pr[4] * f, pr[12] * f, pr[13] * f, pr[5] * f, pr[6] * f);
        FS_HIP(hipMemcpy(pr, d_rctl_f_.as<uint32_t>() + 16, sizeof(pr), hipMemcpyDeviceToHost));
        FS_HIP(hipMemset(d_rctl_f_.as<uint32_t>() + 16, 0, sizeof(pr)));
        fprintf(stderr, "rows fast prof (us/frame summed over the fast launches, workgroup 0; wait+work): preload %.1f  S1 %.1f+%.1f  S2 %.1f+%.1f  S3 %.1f+%.1f  S4 %.1f+%.1f  head %.1f+%.1f  decision %.1f+%.1f (rows' logits -> argmax / draw %.1f, pick -> next input %.1f)  tail %.1f\n",
                pr[0] * f, pr[9] * f, pr[1] * f, pr[10] * f, pr[2] * f, pr[11] * f, (pr[3] + pr[8]) * f, pr[12] * f, pr[4] * f, pr[13] * f, pr[5] * f, pr[14] * f, (pr[6] + pr[15]) * f, pr[15] * f, pr[6] * f, pr[7] * f);
    }
    // seed -> ChaCha key -> a device RngState.  The copy is asynchronous and reads `host`: the caller's, alive until the stream has been waited for
    void upload_rng(uint64_t seed, RngState& host, RngState* dst, hipStream_t st) {
        host = rng_fresh(seed);
        FS_HIP(hipMemcpyAsync(dst, &host, sizeof(host), hipMemcpyHostToDevice, st));
    }
    // one prompt [C + 1][L] left-padded with <|im_end|>/0 to Lmax columns (static_batch.rs:68-111; the pad mask is built but never applied,
    // dual_ar.rs:589-615)
    void left_pad(const uint32_t* prompt, int L, int Lmax, uint32_t* out) const {
        const int C1 = a_.num_codebooks + 1, pad = Lmax - L;
        for (int r = 0; r < C1; ++r) {
            for (int j = 0; j < pad; ++j) out[(size_t)r * Lmax + j] = r == 0 ? t_.im_end_id : 0u;
            std::memcpy(&out[(size_t)r * Lmax + pad], prompt + (size_t)r * L, sizeof(uint32_t) * L);
        }
    }
    // the results of rows [0, n) of a row-path call (hs: their final states): codes [n][C][cap] out of the staging buffer, frame counts,
    // KV lengths -> frames of all rows
    uint64_t copy_out_rows(const std::vector<SeqState>& hs, int n, uint32_t* codes_out, size_t cap, size_t* n_frames) {
        const int C = a_.num_codebooks;
        std::vector<uint32_t> tmp((size_t)n * C * out_cap_);
        FS_HIP(hipMemcpy(tmp.data(), d_out_.p, sizeof(uint32_t) * tmp.size(), hipMemcpyDeviceToHost));
        uint64_t total = 0;
        for (int i = 0; i < n; ++i) {
            const size_t nb = (size_t)hs[i].n_out;
            FS_REQUIRE(nb <= cap, "codes_out capacity too small for the generated frames");
            for (int c = 0; c < C; ++c)
                std::memcpy(codes_out + ((size_t)i * C + c) * cap, tmp.data() + ((size_t)i * C + c) * out_cap_, sizeof(uint32_t) * nb);
            n_frames[i] = nb;
            total += nb;
            seq_len_[i] = hs[i].pos;
        }
        return total;
    }
    // the fast decoder of request rows [0, top): one launch per group of <= PR_FAST_ROWS rows, the last group on the smallest instantiation
    // that holds its rows (top = 5: 4 + 1 rows, top = 6: 4 + 2)
    void launch_rows_fast_groups(int top, bool sampled) {
        for (int r0 = 0; r0 < top; r0 += PR_FAST_ROWS) {
            const int left = std::min(PR_FAST_ROWS, top - r0), Rf = left >= 3 ? 4 : left;
            launch_rows_fast(rows_fast_args(r0, Rf), Rf, sampled, st_);
        }
    }
    // use_persist_ / use_pslow_ / persist_sampled_ select graphs and sampler folding for generate(); a row-path call sets them for its own
    // launches and must leave them cleared however it ends
    struct PersistFlagsGuard {
        LM& lm;
        ~PersistFlagsGuard() { lm.use_persist_ = lm.use_pslow_ = false; }
    };
    void require_loaded() { FS_REQUIRE(loaded_, "weights not loaded: call fs_lm_load_safetensors or fs_lm_load_synthetic first"); }

    // the handle's token layout as the shared sampler setup (lm_kernels.h) takes it
    TokenLayout layout() const { return TokenLayout{t_.im_end_id, t_.pad_id, t_.semantic_start_id, t_.semantic_end_id, t_.has_semantic_end != 0}; }
    // base_cfg() + one request's sampler settings; the callers set what differs (rep_pen = 1 in the batch paths, session, batch_*)
    SampleCfg make_cfg(const fs_sampling& s, uint32_t flags) const {
        return sample_cfg_make(layout(), s.temp, s.top_p, s.top_k, s.repetition_penalty, (flags & FS_GEN_IGNORE_EOS) != 0);
    }
    // Iteration budget of a request of L_total prompt positions behind n_cached cached ones: the prefill iteration + one per k with
    // L_total + k - 1 <= max_new (single_batch.rs:61,77,193-197; static_batch.rs:122,262-267), clamped to the iterations that fit the RoPE
    // table / KV.  generate and the static batch fail on a clamped budget unless the generator ended by itself (the reference fails at
    // dual_ar.rs:623-624); session slots and request rows stop there.
    struct Budget { long long n_iter; bool clamped; };
    Budget iter_budget(long long max_new, long long L_total, long long n_cached = 0) const {
        Budget b{1 + std::max<long long>(0, max_new - L_total + 1), false};
        const long long room = (long long)a_.max_seq_len - (n_cached + L_total) + 1;
        if (b.n_iter > room) { b.n_iter = room; b.clamped = true; }
        FS_REQUIRE(b.n_iter <= out_cap_, "generation longer than the output staging buffer");
        return b;
    }
    SampleCfg base_cfg() const { return sample_cfg_base(layout()); }

    void validate_tokens(const uint32_t* toks, size_t, int B, int L) {
        const int C1 = a_.num_codebooks + 1;
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < C1; ++r)
                for (int l = 0; l < L; ++l) {
                    const uint32_t v = toks[((size_t)b * C1 + r) * L + l];
                    if (r == 0) { if (v >= (uint32_t)a_.vocab_size) throw Error("token id out of vocabulary (index_select out of range)"); }
                    else if (v >= (uint32_t)a_.codebook_size) throw Error("codebook id out of range (index_select out of range)");
                }
    }

    // ---- tensor plan: names/shapes of the reference loader (dual_ar.rs:125-156,219-223,415-419,466-511)
    void plan_tensors() {
        size_t off = 0;
        auto align = [&](size_t v) { return (v + 255) & ~(size_t)255; };
        auto mat = [&](const std::string& name, int64_t rows, int64_t cols, int mul, int roff, std::pair<size_t, size_t> at) {
            tensors_.push_back({name, rows, cols, false, false, at.first, at.second, mul, roff, 0.f, 0.02});  // initializer_range (dual_ar.rs:93)
        };
        auto emb = [&](const std::string& name, int64_t rows, int64_t cols) {
            size_t at = off;
            off = align(off + (size_t)rows * cols * sizeof(KT));
            tensors_.push_back({name, rows, cols, false, true, at, 0, 1, 0, 0.f, 0.02});
            return at;
        };
        // matrix slab (+ per-row f32 scale slab for fp8 weights): {weights offset, scales offset}
        auto slab = [&](int64_t rows, int64_t cols) {
            std::pair<size_t, size_t> at{off, 0};
            off = align(off + (size_t)rows * cols * sizeof(WT));
            if (kFp8) { at.second = off; off = align(off + (size_t)rows * sizeof(float)); }
            return at;
        };
        auto vec = [&](const std::string& name, int64_t n) {
            size_t at = off;
            off = align(off + (size_t)n * sizeof(float));
            tensors_.push_back({name, 1, n, true, false, at, 0, 1, 0, 1.0f, 0.1});
            return at;
        };
        const int64_t D = a_.dim, I = a_.intermediate_size, V = a_.vocab_size;
        const int64_t QKV = (int64_t)(a_.n_head + 2 * a_.n_local_heads) * a_.head_dim;
        o_tok_emb_ = emb("embeddings.weight", V, D);
        o_cb_emb_ = emb("codebook_embeddings.weight", (int64_t)a_.codebook_size * a_.num_codebooks, D);
        auto blocks = [&](int n, const std::string& pre, std::vector<std::array<size_t, 10>>& offs) {
            for (int l = 0; l < n; ++l) {
                const std::string p = pre + std::to_string(l) + ".";
                std::array<size_t, 10> o;
                auto s0 = slab(QKV, D); mat(p + "attention.wqkv.weight", QKV, D, 1, 0, s0);
                auto s1 = slab(D, D); mat(p + "attention.wo.weight", D, D, 1, 0, s1);
                auto s2 = slab(2 * I, D);
                mat(p + "feed_forward.w1.weight", I, D, 2, 0, s2);
                mat(p + "feed_forward.w3.weight", I, D, 2, 1, s2);
                auto s3 = slab(D, I); mat(p + "feed_forward.w2.weight", D, I, 1, 0, s3);
                o[0] = s0.first; o[1] = s1.first; o[2] = s2.first; o[3] = s3.first;
                o[4] = vec(p + "ffn_norm.weight", D);
                o[5] = vec(p + "attention_norm.weight", D);
                o[6] = s0.second; o[7] = s1.second; o[8] = s2.second; o[9] = s3.second;
                offs.push_back(o);
            }
        };
        blocks(a_.n_layer, "layers.", o_slow_);
        o_norm_ = vec("norm.weight", D);
        // tied head (dual_ar.rs:482-486): the embedding table itself, except with fp8 matrices, where the head is the fp8
        // quantisation of the same checkpoint tensor (the table stays bf16 for the lookups)
        if (a_.tie_word_embeddings && !kFp8) o_out_ = {o_tok_emb_, 0};
        else { o_out_ = slab(V, D); mat(a_.tie_word_embeddings ? "embeddings.weight" : "output.weight", V, D, 1, 0, o_out_); }
        o_fast_emb_ = emb("fast_embeddings.weight", a_.codebook_size, D);
        blocks(a_.n_fast_layer, "fast_layers.", o_fast_);
        o_fast_norm_ = vec("fast_norm.weight", D);
        o_fast_out_ = slab(a_.codebook_size, D); mat("fast_output.weight", a_.codebook_size, D, 1, 0, o_fast_out_);
        arena_bytes_ = off;
    }

    void alloc_runtime() {
        arena_.alloc(arena_bytes_);
        uint8_t* base = arena_.as<uint8_t>();
        auto lw = [&](const std::array<size_t, 10>& o) {
            LayerW w;
            w.wqkv = base + o[0]; w.wo = base + o[1]; w.w13 = base + o[2]; w.w2 = base + o[3];
            w.ffn_norm = (const float*)(base + o[4]); w.attn_norm = (const float*)(base + o[5]);
            if (kFp8) {
                w.s_qkv = (const float*)(base + o[6]); w.s_o = (const float*)(base + o[7]);
                w.s_13 = (const float*)(base + o[8]); w.s_2 = (const float*)(base + o[9]);
            }
            return w;
        };
        for (auto& o : o_slow_) slow_.push_back(lw(o));
        for (auto& o : o_fast_) { fast_.push_back(lw(o)); fast_.back().cache_resident = getenv("FISHRT_FAST_NT") == nullptr; }
        tok_emb_ = base + o_tok_emb_; cb_emb_ = base + o_cb_emb_; fast_emb_ = base + o_fast_emb_;
        out_w_ = base + o_out_.first; fast_out_w_ = base + o_fast_out_.first;
        if (kFp8) { out_s_ = (const float*)(base + o_out_.second); fast_out_s_ = (const float*)(base + o_fast_out_.second); }
        norm_w_ = (const float*)(base + o_norm_); fast_norm_w_ = (const float*)(base + o_fast_norm_);
        // RoPE tables on the host exactly as precompute_freqs_cis (dual_ar.rs:168-186): f32 powf / cos / sin
        const int half = a_.head_dim / 2, n_elem = a_.dim / a_.n_head;
        std::vector<float> ct((size_t)a_.max_seq_len * half), sn((size_t)a_.max_seq_len * half), theta(half);
        for (int j = 0; j < half; ++j) theta[j] = 1.f / std::pow(a_.rope_base, (float)(2 * j) / (float)n_elem);
        for (int p = 0; p < a_.max_seq_len; ++p)
            for (int j = 0; j < half; ++j) {
                const float ang = (float)p * theta[j];
                ct[(size_t)p * half + j] = std::cos(ang);
                sn[(size_t)p * half + j] = std::sin(ang);
            }
        d_cos_.alloc(ct.size() * 4); d_sin_.alloc(sn.size() * 4);
        FS_HIP(hipMemcpy(d_cos_.p, ct.data(), ct.size() * 4, hipMemcpyHostToDevice));
        FS_HIP(hipMemcpy(d_sin_.p, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
        // paged KV: one pool per slow layer, page = KV_PAGE tokens x Hk heads x Dh
        // (the table covers whole attention chunks: k_attn_decode reads the slot of every launched chunk unconditionally)
        n_chunks_ = (a_.max_seq_len + AttnKernels<WT>::chunk() - 1) / AttnKernels<WT>::chunk();
        FS_REQUIRE(n_chunks_ <= 128, "max_seq_len too large for the attention chunking (128 chunks)");
        max_pages_ = std::max((a_.max_seq_len + KV_PAGE - 1) / KV_PAGE, n_chunks_ * AttnKernels<WT>::chunk() / KV_PAGE);
        n_pages_ = max_pages_ * B_;
        page_elems_ = (size_t)a_.n_local_heads * KV_PAGE * a_.head_dim;
        // pools and partial buffers start zeroed: the attention kernels read rows / chunks past the current length
        // unconditionally and mask them afterwards, which needs finite (not uninitialised) contents
        kv_pool_.alloc((size_t)a_.n_layer * 2 * n_pages_ * page_elems_ * sizeof(KT));
        FS_HIP(hipMemset(kv_pool_.p, 0, kv_pool_.n));
        d_page_table_.alloc(sizeof(int) * (size_t)std::max(2 * B_ + 1, PR_MAX_ROWS) * max_pages_);  // + the staging rows of a session's joining requests (one group pass)
        FS_HIP(hipMemset(d_page_table_.p, 0, d_page_table_.n));
        pages_.init(n_pages_, B_, KV_PAGE, a_.max_seq_len);
        seq_len_.assign(B_, 0);
        fast_len_.assign(B_, 0);
        // fast-decoder KV: one page per (layer, sequence); its page table is a single zero
        fast_pool_.alloc((size_t)std::max(1, a_.n_fast_layer) * 2 * B_ * page_elems_ * sizeof(KT));
        FS_HIP(hipMemset(fast_pool_.p, 0, fast_pool_.n));
        d_zero_table_.alloc(sizeof(int) * 4);
        FS_HIP(hipMemset(d_zero_table_.p, 0, d_zero_table_.n));
        // activations / state
        // (>= PR_MAX_ROWS rows / states: a request-row launch covers 2, 4 or 8 rows whatever max_batch is -- the padding rows are read, found terminated and skipped)
        d_x_.alloc(sizeof(float) * (size_t)std::max(B_, PR_MAX_ROWS) * a_.dim);
        d_xf_.alloc(sizeof(float) * (size_t)std::max(B_, PR_MAX_ROWS) * a_.dim);
        FS_HIP(hipMemset(d_x_.p, 0, d_x_.n));
        d_q_.alloc(sizeof(float) * a_.dim);
        d_part_.alloc(sizeof(float) * (size_t)a_.n_head * n_chunks_ * (a_.head_dim + 2));
        FS_HIP(hipMemset(d_part_.p, 0, d_part_.n));
        d_act_.alloc(sizeof(float) * a_.intermediate_size);
        d_logits_slow_.alloc(sizeof(float) * a_.vocab_size);
        d_logits_fast_.alloc(sizeof(float) * a_.codebook_size);
        d_hid_slot_.alloc(sizeof(float*));
        FS_HIP(hipMemset(d_hid_slot_.p, 0, sizeof(float*)));
        d_state_.alloc(sizeof(SeqState) * (std::max(B_, PR_MAX_ROWS) + 1));  // + the staging state of a session's joining request (index B_)
        FS_HIP(hipMemset(d_state_.p, 0, d_state_.n));
        d_cfg_.alloc(sizeof(SampleCfg));
        SampleCfg c = base_cfg();
        FS_HIP(hipMemcpy(d_cfg_.p, &c, sizeof(c), hipMemcpyHostToDevice));
        d_rng_.alloc(sizeof(RngState));
        main_.prompt.alloc(sizeof(uint32_t) * (size_t)(a_.num_codebooks + 1) * a_.max_seq_len);
        out_cap_ = a_.max_seq_len + 8;
        d_out_.alloc(sizeof(uint32_t) * (size_t)B_ * a_.num_codebooks * out_cap_);
        rp_.alloc(1, a_.num_codebooks, a_.codebook_size);
        FS_HIP(hipHostMalloc(&h_pin_, 4096, hipHostMallocDefault));
    }

    // rows of output.weight read by the generator's slow head: [im_end, V) for Fish 1.5 (utils.rs:13-16); the gathered
    // {pad_id, im_end_id} pair for Fish <= 1.4
    const void* slow_head_w() {
        if (!legacy_ && !generic_) return (const uint8_t*)out_w_ + (size_t)t_.im_end_id * a_.dim * sizeof(WT);
        if (!d_legacy_head_.p) d_legacy_head_.alloc(gathered_head_bytes() + sizeof(float) * n_audio_ + 256);
        return d_legacy_head_.p;
    }
    size_t gathered_head_bytes() const { return ((sizeof(WT) * (size_t)n_audio_ * a_.dim) + 15) & ~(size_t)15; }
    // per-row scales of the same rows (fp8 weights only)
    const float* slow_head_s() {
        if (!kFp8) return nullptr;
        if (!legacy_ && !generic_) return out_s_ + t_.im_end_id;
        slow_head_w();
        return (const float*)(d_legacy_head_.as<uint8_t>() + gathered_head_bytes());
    }
    void refresh_legacy_head() {
        if (generic_) {  // [W[im_end]; W[semantic_start .. V)]
            const size_t row = sizeof(WT) * (size_t)a_.dim;
            uint8_t* dst = (uint8_t*)const_cast<void*>(slow_head_w());
            FS_HIP(hipMemcpyAsync(dst, (const uint8_t*)out_w_ + t_.im_end_id * row, row, hipMemcpyDeviceToDevice, st_));
            FS_HIP(hipMemcpyAsync(dst + row, (const uint8_t*)out_w_ + t_.semantic_start_id * row, row * (n_audio_ - 1), hipMemcpyDeviceToDevice, st_));
            if (kFp8) {
                float* ds = const_cast<float*>(slow_head_s());
                FS_HIP(hipMemcpyAsync(ds, out_s_ + t_.im_end_id, sizeof(float), hipMemcpyDeviceToDevice, st_));
                FS_HIP(hipMemcpyAsync(ds + 1, out_s_ + t_.semantic_start_id, sizeof(float) * (n_audio_ - 1), hipMemcpyDeviceToDevice, st_));
            }
            FS_HIP(hipStreamSynchronize(st_));
            return;
        }
        if (!legacy_) return;
        launch_gather_rows<WT>(out_w_, a_.dim, t_.pad_id, t_.im_end_id, const_cast<void*>(slow_head_w()), st_);
        if (kFp8) launch_gather_rows<float>(out_s_, 1, t_.pad_id, t_.im_end_id, const_cast<float*>(slow_head_s()), st_);
        FS_HIP(hipStreamSynchronize(st_));
    }
    SeqState* state(int b) { return d_state_.as<SeqState>() + b; }
    float* x(int b) { return d_x_.as<float>() + (size_t)b * a_.dim; }
    float* xf(int b) { return d_xf_.as<float>() + (size_t)b * a_.dim; }
    KVView slow_kv(int layer, int b) {
        KVView v;
        KT* base = kv_pool_.as<KT>() + (size_t)layer * 2 * n_pages_ * page_elems_;
        v.k = base; v.v = base + (size_t)n_pages_ * page_elems_;
        v.page_table = d_page_table_.as<int>() + (size_t)b * max_pages_;
        return v;
    }
    KVView fast_kv(int layer, int b) {
        KVView v;
        KT* base = fast_pool_.as<KT>() + ((size_t)layer * 2 * B_) * page_elems_;
        v.k = base + (size_t)b * page_elems_;
        v.v = base + ((size_t)B_ + b) * page_elems_;
        v.page_table = d_zero_table_.as<int>();
        return v;
    }

    // ---- KV paging (host side; the device only ever sees the page table)
    // Who holds which page is the book's business (fs_kv_pages.h: pages are reference counted -- a session's shared prefix pages have the
    // prefix + every slot on it as owners -- and outside sessions every page has one owner); the engine uploads rows and counts tokens.
    void ensure_capacity(int b, int n_tokens) {
        if (!pages_.grow(b, n_tokens)) return;
        upload_row(b, st_, pages_.of(b));
        FS_HIP(hipStreamSynchronize(st_));  // the list may be reallocated by the next call
    }
    void truncate(int b, int pos) {  // keep the first `pos` tokens (dual_ar.rs:392-404)
        pages_.truncate(b, pos);
        seq_len_[b] = pos;
    }
    // the one copy of page ids into the device's page table, from its row `row` on (rows >= B_: the staging rows of a joining pass), on
    // stream st: a sequence's or a prefix's list, the scratch page of a parked slot, or the rows of a group pass side by side.  The
    // source must outlive the copy.
    void upload_row(int row, hipStream_t st, const int* ids, size_t n) {
        FS_HIP(hipMemcpyAsync(d_page_table_.as<int>() + (size_t)row * max_pages_, ids, sizeof(int) * n, hipMemcpyHostToDevice, st));
    }
    void upload_row(int row, hipStream_t st, const std::vector<int>& ids) { upload_row(row, st, ids.data(), ids.size()); }

    // Runs the next `n` prompt tokens (columns state->step ..) of the staged prompt through the slow transformer,
    // appending their K/V.  Afterwards x(b) holds the pre-norm hidden state of the last processed token.
    void prefill_tokens(int b, int n, bool use_graph) {
        if (n <= 0) return;
        if (RowKernels<WT>::has_mfma_prefill() && n > 1 && a_.dim % 128 == 0 && a_.intermediate_size % 128 == 0) {
            ensure_prefill_buffers();
            const int M = launch_seq_pass(main_, state(b), b, seq_len_[b], n);
            FS_HIP(hipMemcpyAsync(x(b), main_.x.as<float>() + (size_t)(M - 1) * a_.dim, sizeof(float) * a_.dim, hipMemcpyDeviceToDevice, st_));
            return;
        }
        for (int l = 0; l < n; ++l) {
            set_bucket(seq_len_[b] + l + 1);
            if (use_graph && b == 0) { use_graphs_for_bucket(); FS_HIP(hipGraphLaunch(g_step_, st_)); continue; }
            LmKernels<WT>::embed(d_, tok_emb_, cb_emb_, a_.num_codebooks, a_.codebook_size, d_cfg_.as<SampleCfg>(),
                                 main_.prompt.as<uint32_t>(), state(b), x(b), st_);
            enqueue_slow_layers(b);
            launch_advance(state(b), st_);
        }
    }
    // One sequence's next n prompt tokens -- the columns state->step .. of the lane's staged prompt, at positions start .. -- through the
    // slow transformer on the lane's stream, in passes of the row buffers' capacity; their K/V go to page-table row kv_row.  Returns the
    // rows of the last pass: row M - 1 of the lane's x then holds the pre-norm hidden state of the last token.
    int launch_seq_pass(PrefillLane& ln, SeqState* st, int kv_row, int start, int n) {
        RowsCtx c = ln.ctx(st, /*pos_step=*/1, /*pt_stride=*/0);
        int M = 0;
        for (int done = 0; done < n; done += M) {
            M = std::min(a_.head_dim == 64 ? kRowsCap : kPartRows, n - done);
            c.nc_launch = chunk_bucket(start + done + M);
            RowKernels<WT>::prefill_embed(d_, tok_emb_, cb_emb_, a_.num_codebooks, a_.codebook_size, d_cfg_.as<SampleCfg>(),
                                         ln.prompt.as<uint32_t>(), st, M, ln.x.as<float>(), ln.st);
            for (int l = 0; l < a_.n_layer; ++l) RowKernels<WT>::rows_layer(d_, M, c, slow_[l], slow_kv(l, kv_row), l == 0, ln.st);
            RowKernels<WT>::rows_finish(d_, M, c, nullptr, ln.st);
            launch_advance_n(st, M, ln.st);
        }
        return M;
    }
    // ONE group pass on the lane's stream: S sequences of Lp rows each side by side (prompts: device [S][pstride], C + 1 rows of Lp columns
    // per sequence), K/V into the page-table rows kv_row ..; seq_states (device [S], or null: all at st->pos) gives each its first position,
    // nc_launch the attention chunks that cover the longest
    void launch_group_pass(PrefillLane& ln, const uint32_t* prompts, int S, int Lp, size_t pstride, SeqState* st, int kv_row,
                           const SeqState* seq_states, int nc_launch) {
        RowsCtx c = ln.ctx(st, /*pos_step=*/1, /*pt_stride=*/max_pages_);
        c.seq_rows = Lp;
        c.nc_launch = nc_launch;
        c.seq_states = seq_states;
        const int M = S * Lp;
        RowKernels<WT>::prefill_embed(d_, tok_emb_, cb_emb_, a_.num_codebooks, a_.codebook_size, d_cfg_.as<SampleCfg>(), prompts, st, M,
                                     ln.x.as<float>(), ln.st, Lp, pstride);
        for (int l = 0; l < a_.n_layer; ++l) RowKernels<WT>::rows_layer(d_, M, c, slow_[l], slow_kv(l, kv_row), l == 0, ln.st);
    }
    void ensure_prefill_buffers() {
        if (main_.x.p) return;
        const int I = a_.intermediate_size;
        down_split_ = I % 1024 == 0 ? I / 1024 : (I % 256 == 0 ? I / 256 : I / 128);
        main_.ensure(a_, down_split_, n_chunks_, d_cos_.as<float>(), d_sin_.as<float>());
    }
    // the in-launch split-K sums of the folded decode steps give up after ~0.1 s of polling (a tile's blocks were not co-resident): loud failure
    void check_rows_xchg() {
        if (!d_epoch_.p) return;
        uint32_t e[2] = {0, 0};
        FS_HIP(hipMemcpy(e, d_epoch_.p, sizeof(e), hipMemcpyDeviceToHost));
        if (e[1] != 0) {
            const uint32_t z = 0;
            FS_HIP(hipMemcpy(d_epoch_.as<uint32_t>() + 1, &z, sizeof(z), hipMemcpyHostToDevice));
            // this call's tokens are garbage (reported), but the handle recovers: the folded step is off from now on and the captured step
            // graphs are dropped, so the next call runs the slab + k_prep step instead of timing out again
            fold_off_ = true;
            drop_batch_graphs();
            throw Error("static-batch decode: " + std::to_string(e[1]) + " split-K exchange waits timed out (a down projection's blocks were not co-resident); "
                        "this handle falls back to the slab path for its next calls");
        }
    }
    void ensure_batch_buffers() {
        if (d_xfrows_.p) return;
        ld_slow_ = ((n_audio_ + 63) / 64) * 64;
        d_xfrows_.alloc(sizeof(float) * kRows * a_.dim);
        d_lrows_.alloc(sizeof(float) * kRows * ld_slow_);
        d_lfast_.alloc(sizeof(float) * kRows * a_.codebook_size);
        std::vector<SeqState> fs(8);
        for (int i = 0; i < 8; ++i) { fs[i] = SeqState{}; fs[i].pos = i; }
        d_fast_state_.alloc(sizeof(SeqState) * 8);
        FS_HIP(hipMemcpy(d_fast_state_.p, fs.data(), sizeof(SeqState) * 8, hipMemcpyHostToDevice));
        std::vector<int> tb(B_);
        for (int i = 0; i < B_; ++i) tb[i] = i;
        d_rwords_.alloc(sizeof(uint32_t) * 16 * kRows);
        // folded decode steps (k_gemm_down): exchange units of the in-launch split-K sums + {step epoch, timeouts}
        d_xchg_.alloc(rows_xchg_bytes(a_.dim));
        FS_HIP(hipMemset(d_xchg_.p, 0, d_xchg_.n));
        d_epoch_.alloc(sizeof(uint32_t) * 2);
        const uint32_t e0[2] = {1u, 0u};
        FS_HIP(hipMemcpy(d_epoch_.p, e0, sizeof(e0), hipMemcpyHostToDevice));
        d_fast_table_.alloc(sizeof(int) * B_);
        FS_HIP(hipMemcpy(d_fast_table_.p, tb.data(), sizeof(int) * B_, hipMemcpyHostToDevice));
        hid_.dev.alloc(sizeof(HidSlot) * B_);
        FS_HIP(hipMemset(hid_.dev.p, 0, hid_.dev.n));
        sc_.dev.alloc(sizeof(ScoreSlot) * B_);
        FS_HIP(hipMemset(sc_.dev.p, 0, sc_.dev.n));
    }
    // one static-batch frame for B rows: x rows (main_.x) hold the embedded inputs of position state(0)->pos
    void enqueue_batch_frame(int B) {
        const int C = a_.num_codebooks;
        // lock-step static batch: every row at state(0)->pos (left-padded prompts); session: row m is its own sequence at state(m)->pos
        RowsCtx cs = main_.ctx(state(0), /*pos_step=*/sess_active_ ? -1 : 0, /*pt_stride=*/max_pages_);
        cs.nc_launch = nc_launch_;
        // decode steps of <= 32 rows: the down projections close every layer themselves (in-launch split-K sums: no slabs, no k_prep nodes but the first)
        cs.xchg = d_xchg_.p; cs.epoch = d_epoch_.as<uint32_t>();
        const bool fold = !fold_off_ && RowKernels<WT>::rows_fold_ok(d_, B, cs) && a_.n_layer <= 64 && a_.n_fast_layer <= 8 && C <= 32;
        cs.fold = fold;
        for (int l = 0; l < a_.n_layer; ++l, cs.node_id = (uint32_t)l)
            RowKernels<WT>::rows_layer(d_, B, cs, slow_[l], slow_kv(l, 0), l == 0, st_, fold ? (l + 1 < a_.n_layer ? slow_[l + 1].attn_norm : norm_w_) : nullptr);
        if (!fold) RowKernels<WT>::rows_finish(d_, B, cs, norm_w_, st_);
        RowKernels<WT>::rows_head(d_, B, cs, slow_head_w(), slow_head_s(), n_audio_, d_lrows_.as<float>(), ld_slow_, st_, fold);
        // session steps: the collecting slots' hidden-state rows (one node behind the slow head; null table entries exit at once, so the
        // one captured graph serves every mix of collecting and non-collecting slots)
        if (sess_active_) launch_hidden_rows(hid_.dev.as<HidSlot>(), state(0), cs.X, a_.dim, B, st_);
        // block-parallel samplers (temp > 1e-7, top_k <= 256): the step's C + 1 StdRng words per row are derived up front
        const bool slots = sess_.slots;  // FS_SESSION_PER_SLOT: the 9 sampler nodes are the per-slot ones, one for one
        const uint32_t* words = rows_par_ ? d_rwords_.as<uint32_t>() : nullptr;
        if (rows_par_) SampleKernels<WT>::rows_rng_words(d_rng_.as<RngState>(), B, C + 1, state(0), d_rwords_.as<uint32_t>(), st_);
        const bool capt = cap_frames_ > 0 && d_rcap_.p && d_rcap_.n >= sizeof(float) * (size_t)B * cap_frames_ * 9 * 2048;  // (fs_lm_debug_capture)
        if (capt) launch_cap_rows_logits(d_lrows_.as<float>(), ld_slow_, n_audio_, state(0), d_cfg_.as<SampleCfg>(), B, d_rcap_.as<float>(), cap_frames_, 0, st_);
        // folded steps: the sampler that writes a fast-decoder input row also leaves its first layer's normalised GEMM input (no k_prep node)
        const float* prep_g = fold && a_.dim <= 1024 ? fast_[0].attn_norm : nullptr;
        // FS_SESSION_SCORE: one score node in front of each per-slot sampler node, behind the capture of the raw row (null table entries
        // exit at once, so the one captured graph serves every mix of scoring and generating slots)
        const bool score = slots && sess_.score;
        // FS_SESSION_TRACE: the score nodes know the traced slots' stash, and one tail node behind the last sampler closes their rows
        const bool trace = score && sess_.trace;
        float* stash = trace ? d_trace_.as<float>() : nullptr;
        // FS_SESSION_ALTS: the score nodes (and the tail node) are their second instantiation, N a launch argument
        const int alts = score ? sess_.alts : 0;
        if (score) launch_score_slots(sc_.dev.as<ScoreSlot>(), state(0), d_scfg_.as<SampleCfg>(), d_lrows_.as<float>(), ld_slow_, n_audio_, 0, C, B, st_, stash, alts);
        if (slots)
            SampleKernels<WT>::sample_slow_slots(d_, d_lrows_.as<float>(), ld_slow_, n_audio_, d_scfg_.as<SampleCfg>(), d_srng_.as<SlotRng>(), B, state(0),
                                                 cs.X, d_xfrows_.as<float>(), st_, prep_g, cs.A, fold ? d_epoch_.as<uint32_t>() : nullptr,
                                                 capt ? d_rcap_.as<float>() : nullptr, cap_frames_, sess_.wide);
        else
        SampleKernels<WT>::sample_slow_rows(d_, d_lrows_.as<float>(), ld_slow_, n_audio_, d_cfg_.as<SampleCfg>(), d_rng_.as<RngState>(), B,
                                            C + 1, state(0), cs.X, d_xfrows_.as<float>(), st_, words, prep_g, cs.A, fold ? d_epoch_.as<uint32_t>() : nullptr);
        // the fast decoder's context of codebook pass cbi.  Passes 1..: the first fast layer's q / k / v come from the qkv table (row = the code the
        // previous pass picked; no k_prep, no Wqkv node) where rows_layer will take it -- ONE predicate decides the table, the sampler's
        // normalised fragments and first_prepped, so a pass never finds neither the table nor its prepared input
        const bool qkv0_on = fold && d_qkv0_.p && !getenv("FISHRT_ROWS_NO_QKV0") && a_.codebook_size == 1024;
        auto fast_ctx = [&](int cbi) {
            RowsCtx cf = cs;
            cf.X = d_xfrows_.as<float>();
            cf.state = d_fast_state_.as<SeqState>() + cbi;
            cf.pos_step = 0;  // (the fast decoder's rows always sit at codebook position cbi)
            cf.pt_stride = 1;
            cf.nc_launch = 1;
            cf.small_attn = a_.num_codebooks <= 8;
            cf.identity_pages = true;  // d_fast_table_[i] == i
            cf.attn_t1 = cbi == 0;     // d_fast_state_[0].pos == 0
            if (qkv0_on && AttnKernels<WT>::rows_qkv0_ok(d_, cf)) { cf.qkv0_tbl = d_qkv0_.as<float>(); cf.row_states = state(0); cf.code_slot = cbi; }
            return cf;
        };
        RowsCtx cf = fast_ctx(0);
        cf.first_prepped = prep_g != nullptr;  // (left by the slow-token sampler)
        for (int cbi = 0; cbi < C; ++cbi) {
            for (int l = 0; l < a_.n_fast_layer; ++l) {
                KVView kv;
                KT* base = fast_pool_.as<KT>() + ((size_t)l * 2 * B_) * page_elems_;
                kv.k = base; kv.v = base + (size_t)B_ * page_elems_; kv.page_table = d_fast_table_.as<int>();
                cf.node_id = 64u + (uint32_t)cbi * 8u + (uint32_t)l;
                RowKernels<WT>::rows_layer(d_, B, cf, fast_[l], kv, l == 0, st_, fold ? (l + 1 < a_.n_fast_layer ? fast_[l + 1].attn_norm : fast_norm_w_) : nullptr);
            }
            if (!fold) RowKernels<WT>::rows_finish(d_, B, cf, fast_norm_w_, st_);
            RowKernels<WT>::rows_head(d_, B, cf, fast_out_w_, kFp8 ? fast_out_s_ : nullptr, a_.codebook_size, d_lfast_.as<float>(), a_.codebook_size, st_, fold);
            if (capt) launch_cap_rows_logits(d_lfast_.as<float>(), a_.codebook_size, a_.codebook_size, state(0), d_cfg_.as<SampleCfg>(), B, d_rcap_.as<float>(),
                                             cap_frames_, 1 + cbi, st_);
            // the pass that reads this sampler's row: with the qkv table its first layer needs no normalised GEMM input from the sampler
            RowsCtx nf = fast_ctx(cbi + 1);
            const float* prep_f = nf.qkv0_tbl ? nullptr : prep_g;
            nf.first_prepped = prep_f != nullptr;
            if (score) launch_score_slots(sc_.dev.as<ScoreSlot>(), state(0), d_scfg_.as<SampleCfg>(), d_lfast_.as<float>(), a_.codebook_size, a_.codebook_size,
                                          1 + cbi, C, B, st_, stash, alts);
            if (slots) {
                RepPenState rp0 = srp_.view(0);
                SampleKernels<WT>::sample_fast_slots(d_, d_lfast_.as<float>(), cbi, C, a_.codebook_size, d_scfg_.as<SampleCfg>(), d_srng_.as<SlotRng>(), rp0,
                                                     B, state(0), fast_emb_, d_xfrows_.as<float>(), tok_emb_, cb_emb_, cs.X, d_out_.as<uint32_t>(), out_cap_,
                                                     st_, prep_f, cs.A, sess_.wide);
            } else
            SampleKernels<WT>::sample_fast_rows(d_, d_lfast_.as<float>(), cbi, C, a_.codebook_size, d_cfg_.as<SampleCfg>(),
                                                d_rng_.as<RngState>(), B, state(0), fast_emb_, d_xfrows_.as<float>(), tok_emb_, cb_emb_,
                                                cs.X, d_out_.as<uint32_t>(), out_cap_, st_, words, prep_f, cs.A);
            cf = nf;
        }
        if (trace) launch_trace_commit(sc_.dev.as<ScoreSlot>(), state(0), d_scfg_.as<SampleCfg>(), stash, n_audio_, a_.codebook_size, C, B, st_, alts);
        if (capt) launch_cap_rows_picks(state(0), d_cfg_.as<SampleCfg>(), B, d_rcap_.as<float>(), cap_frames_, C, st_);
    }
    // the capture record of a row-path call: [B][cap_frames][9][2048] (allocated when fs_lm_debug_capture is armed)
    void ensure_rows_capture(int B) {
        if (!cap_frames_) return;
        FS_REQUIRE((size_t)B * cap_frames_ <= 4096, "decision capture on the row path: rows x frames limited to 4096 (302 MB)");
        d_rcap_.alloc(sizeof(float) * (size_t)B * cap_frames_ * 9 * 2048);
        FS_HIP(hipMemsetAsync(d_rcap_.p, 0, d_rcap_.n, st_));
    }
    void drop_batch_graphs() {
        for (auto& kv : batch_graphs_) if (kv.second) (void)hipGraphExecDestroy(kv.second);
        batch_graphs_.clear();
    }
    void destroy_graphs() {  // every captured graph of the handle
        for (auto& kv : graphs_)
            for (hipGraphExec_t g : {kv.second.first, kv.second.second}) if (g) (void)hipGraphExecDestroy(g);
        graphs_.clear();
        for (auto& kv : multi_graphs_) if (kv.second) (void)hipGraphExecDestroy(kv.second);
        multi_graphs_.clear();
        g_frame_ = g_step_ = nullptr;
        drop_batch_graphs();
    }
    hipGraphExec_t batch_graph(int B) {
        // (FS_SESSION_ALTS: N is an argument of the captured nodes, so it is part of the key -- bits 32 and up, 0 without the flag)
        const long long key = (sess_active_ ? 1 << 24 : 0) + (rows_par_ ? 1 << 25 : 0) + (sess_.slots ? 1 << 26 : 0) + (sess_.slots && sess_.wide ? 1 << 27 : 0) +
                              (sess_.slots && sess_.score ? 1 << 28 : 0) + (sess_.slots && sess_.score && sess_.trace ? 1 << 29 : 0) + B * 1024 + nc_launch_ +
                              ((long long)(sess_.slots && sess_.score ? sess_.alts : 0) << 32);
        auto it = batch_graphs_.find(key);
        if (it != batch_graphs_.end()) return it->second;
        {   // the co-residency query of the folded step (rows_fold_ok -> occupancy API) is answered once, OUTSIDE stream capture
            RowsCtx cs = main_.ctx(state(0), 0, max_pages_);
            cs.xchg = d_xchg_.p; cs.epoch = d_epoch_.as<uint32_t>();
            (void)RowKernels<WT>::rows_fold_ok(d_, B, cs);
        }
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        FS_HIP(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
        enqueue_batch_frame(B);
        FS_HIP(hipStreamEndCapture(st_, &g));
        FS_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        FS_HIP(hipGraphDestroy(g));
        batch_graphs_[key] = ge;
        return ge;
    }

    // naps before the first sweep of each stage kind (64-clock units; tuned on MI355X, profiles/r03_poll_naps.txt); the environment
    // variables ("a,b,c,d,e,f") override them for tuning runs
    static constexpr int kNapsFast[6] = {16, 16, 16, 16, 16, 16}, kNapsSlow[6] = {20, 16, 6, 36, 36, 12};  // (round 6, behind the layer-0 qkv table: 530.0 -> 528.4 us, profiles/r06_tune_naps.txt)
    // (re-tuned in round 5 behind the publishing-wave epilogues and the early W13 request: 558.8 -> 551.1 us on the tuner's workload; again at the end of the round: 543.1 -> 542.2, and behind the matrix-core S4 of the slow kernel: 541.9 -> 540.3)
    // the same coordinate descent on the in-launch-sampler instantiation of k_fast_persist (680 -> 662 us per sampled frame) and on the
    // e4m3 image of k_slow_persist (595 -> 585 us per fp8 frame): their stage arithmetic differs, so the edges complete at other times
    static constexpr int kNapsFastSampled[6] = {12, 16, 12, 20, 12, 16}, kNapsSlowFp8[6] = {20, 4, 28, 24, 24, 0};  // (round 5 re-tune: profiles/r05_tune_naps.txt)
    // default stream policy of k_slow_persist per dtype, decided by same-box interleaved A/B (profiles/slow_stream_policy_ab.txt: bf16
    // 525.2 -> 513.4 us per frame, fp8 531.5 -> 519.7, five interleaved repetitions, identical tokens)
    static constexpr bool kSlowStreamNt = true, kSlowStreamNtFp8 = true;
    static void set_naps(int (&naps)[6], const char* env, const int (&dflt)[6]) {
        for (int i = 0; i < 6; ++i) naps[i] = dflt[i];
        if (const char* v = getenv(env)) {
            int i = 0;
            for (const char* p = v; *p && i < 6; ++i) { naps[i] = atoi(p); while (*p && *p != ',') ++p; if (*p == ',') ++p; }
        }
    }
    // ---- persistent fast decoder (lm_persist.hip): per-lane weight image, edge buffers, control words
    void pack_persist() {
        persist_ok_ = false;
        // the layer-0 qkv table is a function of the weights: it goes with them (every return below that builds none leaves none), and with it
        // the captured graphs that carry its address
        if (d_qkv0_.p) { destroy_graphs(); d_qkv0_.free(); }
        if constexpr (std::is_same<WT, bf16_t>::value || std::is_same<WT, fp8_t>::value) {
            constexpr bool FP8 = std::is_same<WT, fp8_t>::value;
            if (getenv("FISHRT_NO_PERSIST")) return;
            if (!fast_persist_supported(d_, a_.n_fast_layer, a_.num_codebooks, a_.codebook_size)) return;
            hipDeviceProp_t prop;
            FS_HIP(hipGetDeviceProperties(&prop, device_));
            if (prop.multiProcessorCount < PF_BLOCKS) return;  // every workgroup needs its own CU
            if (!d_pack_.p) {
                d_pack_.alloc(fast_persist_pack_bytes());
                d_edges_.alloc(fast_persist_edge_bytes());
                FS_HIP(hipMemset(d_edges_.p, 0, d_edges_.n));
                d_ctl_.alloc(320);
                FS_HIP(hipMemset(d_ctl_.p, 0, d_ctl_.n));
                if (FP8) d_fscl_.alloc(sizeof(float) * (size_t)PF_BLOCKS * PF_SCL);
            }
            launch_fast_persist_pack(fast_.data(), fast_out_w_, d_pack_.p, st_, FP8, fast_out_s_, d_fscl_.as<float>());
            // layer-0 qkv table of the codebook passes 1..7 (lm_persist.hip: 7 of a frame's 137 stages become three loads per lane)
            if (!getenv("FISHRT_FAST_NO_QKV0")) {
                d_qkv0_.alloc(fast_persist_qkv0_bytes());
                launch_fast_persist_qkv0_table(d_pack_.p, FP8 ? d_fscl_.as<float>() : nullptr, fast_[0].attn_norm, fast_emb_, d_.eps, d_qkv0_.as<float>(), st_);
            }
            FS_HIP(hipStreamSynchronize(st_));
            persist_ok_ = true;
            // slow transformer: same geometry, the audio-range head must fit 8 rows per workgroup
            pslow_ok_ = false;
            if (getenv("FISHRT_NO_PERSIST_SLOW") || n_audio_ > 8 * PF_BLOCKS) return;
            if (const char* c = getenv("FISHRT_SLOW_STREAM"))  // (checked here, outside any capture; pslow_args() reads it)
                FS_REQUIRE(strcmp(c, "default") == 0 || strcmp(c, "nt") == 0, "FISHRT_SLOW_STREAM must be 'default' or 'nt'");
            if (!d_spack_.p) {
                d_spack_.alloc(slow_persist_pack_bytes(a_.n_layer, FP8));
                d_hpack_.alloc((size_t)PF_BLOCKS * PS_HEAD_IMAGE);
                if (FP8) d_sscl_.alloc(sizeof(float) * slow_persist_scale_floats(a_.n_layer));
                d_snorms_.alloc(sizeof(float) * (size_t)(2 * a_.n_layer + 1) * a_.dim);
                d_sedges_.alloc(slow_persist_edge_bytes());
                FS_HIP(hipMemset(d_sedges_.p, 0, d_sedges_.n));
                d_sctl_.alloc(320);
                FS_HIP(hipMemset(d_sctl_.p, 0, d_sctl_.n));
            }
            std::vector<const float*> np;
            for (int l = 0; l < a_.n_layer; ++l) { np.push_back(slow_[l].attn_norm); np.push_back(slow_[l].ffn_norm); }
            np.push_back(norm_w_);
            if (FP8) launch_slow_persist_pack_fp8(slow_.data(), a_.n_layer, slow_head_w(), slow_head_s(), n_audio_, np.data(), d_spack_.p, d_hpack_.p,
                                                  d_sscl_.as<float>(), d_snorms_.as<float>(), st_);
            else launch_slow_persist_pack(slow_.data(), a_.n_layer, slow_head_w(), n_audio_, np.data(), d_spack_.p, d_hpack_.p, d_snorms_.as<float>(), st_);
            FS_HIP(hipStreamSynchronize(st_));
            pslow_ok_ = true;
        }
    }
    SlowPersistArgs pslow_args() {
        SlowPersistArgs A = {};
        A.wpack = d_spack_.p; A.hpack = d_hpack_.p; A.norms = d_snorms_.as<float>();
        A.scales = d_sscl_.p ? d_sscl_.as<float>() : nullptr;
        A.hscales = d_sscl_.p ? d_sscl_.as<float>() + (size_t)a_.n_layer * PF_BLOCKS * 48 : nullptr;
        A.n_layer = a_.n_layer; A.n_head_rows = n_audio_;
        A.cos_t = d_cos_.as<float>(); A.sin_t = d_sin_.as<float>(); A.eps = d_.eps;
        A.x = x(0); A.logits = d_logits_slow_.as<float>(); A.state = state(0);
        A.kv_pool = kv_pool_.p; A.layer_half = (size_t)n_pages_ * page_elems_;
        A.page_table = d_page_table_.as<int>();
        // Token slices per query head.  8 slices = 128 attention workgroups: the other 128 have no attention item and request their W13 slice
        // three stages ahead (k_slow_persist early_mode bit 0), and S3 merges 8 partials per head.  16 slices halve S2's tokens per slice but give
        // every workgroup an item (W13 arrives as one burst again: S4 waits 31 -> 47-49 us per frame) and double S3's sweep: measured per frame
        // at 8 / 16 slices (profiles/r05_kv_slices.txt): KV 1100 568 / 588 us, 2100 587 / 612, 3100 605 / 611, 4100 624 / 629, 6000 646 / 632
        // (fp8: 1100 576 / 583, 2100 594 / 602, 4100 631 / 620) -- 16 only beyond 4096 cached tokens.
        A.n_sl = std::min(nc_launch_, nc_launch_ > 32 ? 16 : 8);
        if (const char* c = getenv("FISHRT_NSL_MAX")) A.n_sl = std::max(1, std::min(A.n_sl, atoi(c)));  // (debug knobs)
        if (const char* c = getenv("FISHRT_NSL_MIN")) A.n_sl = std::min(16, std::max(A.n_sl, atoi(c)));
        while (A.n_sl & (A.n_sl - 1)) A.n_sl &= A.n_sl - 1;  // the kernel's item mapping needs a power of two (10 / 12 slices: grid-wait timeouts)
        // (measured, round 3: half / a quarter as many slices -> S2 +44 / +115 us per frame, S3 only -10 / -12)
        A.edges = d_sedges_.as<unsigned long long>();
        A.ctl = d_sctl_.as<uint32_t>();
        A.prof = getenv("FISHRT_PERSIST_PROF") ? reinterpret_cast<unsigned long long*>(d_sctl_.as<uint32_t>() + 16) : nullptr;
        A.peer_stamps = (A.prof && d_ctl_.p) ? reinterpret_cast<const unsigned long long*>(d_ctl_.as<uint32_t>() + 16) + 16 : nullptr;
        set_naps(A.naps, "FISHRT_NAPS_SLOW", kFp8 ? kNapsSlowFp8 : kNapsSlow);
        A.prof_wg = getenv("FISHRT_PERSIST_PROF_WG") ? atoi(getenv("FISHRT_PERSIST_PROF_WG")) : 0;
        // k_slow_persist early_mode bits.  bit 3 (round 6, bf16 images): an attention workgroup requests its first K/V tile BEHIND S1's publish instead of
        // in front of the Wqkv rows -- the publishing stores used to queue behind the tile's 32 KB of loads in the CU's vector-memory pipeline (S1 work
        // 1.2 -> 0.7 us on those workgroups; 529.3 -> 526.1 us per frame, 614.5 -> 604.6 at 4100 cached tokens; fp8: no difference, left off)
        A.l2_touch = (getenv("FISHRT_SLOW_EARLY") ? atoi(getenv("FISHRT_SLOW_EARLY")) : (kFp8 ? 1 : 9)) & 15;
        // (bits 0..3 only: bit 4 belongs to the stream policy below, higher bits have no meaning)
        // The stream policy of the slow kernel's weight images (PS_STREAM_NT: non-temporal loads of the bytes a CU reads once per frame).  Read here, by
        // the handle that sets up a launch (a graph capture or a direct launch), like the bits above and the naps: two handles of one process can differ,
        // and an A/B sets it before the handle's first call and leaves it.  FISHRT_SLOW_STREAM=default | nt (anything else is refused when the handle
        // packs its images, pack_persist()); without it the per-dtype default.
        bool stream_nt = kFp8 ? kSlowStreamNtFp8 : kSlowStreamNt;
        if (const char* c = getenv("FISHRT_SLOW_STREAM")) stream_nt = strcmp(c, "nt") == 0;
        if (stream_nt) A.l2_touch |= PS_STREAM_NT;
        return A;
    }
    // the persistent fast decoder takes the slow-token decision in its prologue (no k_sample_slow node) whenever it runs
    bool fold_slow_sampler() const { return use_persist_ && n_audio_ <= 2048; }  // (Fish <= 1.4 too: the 2-way {pad, im_end} draw is taken in-launch)
    FastPersistArgs persist_args() {
        FastPersistArgs A = {};
        A.wpack = d_pack_.p;
        A.scales = d_fscl_.p ? d_fscl_.as<float>() : nullptr;
        for (int l = 0; l < PF_LAYERS; ++l) { A.norms[2 * l] = fast_[l].attn_norm; A.norms[2 * l + 1] = fast_[l].ffn_norm; }
        A.norms[2 * PF_LAYERS] = fast_norm_w_;
        A.fast_emb = fast_emb_; A.tok_emb = tok_emb_; A.cb_emb = cb_emb_;
        A.qkv0_tbl = d_qkv0_.p ? d_qkv0_.as<float>() : nullptr;
        A.cos_t = d_cos_.as<float>(); A.sin_t = d_sin_.as<float>();
        A.eps = d_.eps;
        const bool fold = fold_slow_sampler();
        A.xf = fold ? x(0) : xf(0); A.x = x(0);
        A.slow_logits = fold ? d_logits_slow_.as<float>() : nullptr; A.n_slow = n_audio_; A.hid_slot = d_hid_slot_.as<float*>();
        A.cap = d_cap_.as<float>(); A.cap_frames = cap_frames_;
        A.state = state(0); A.cfg = d_cfg_.as<SampleCfg>(); A.rp = rp_.view(0); A.rng = d_rng_.as<RngState>();
        A.out_codes = d_out_.as<uint32_t>(); A.out_cap = out_cap_;
        A.edges = d_edges_.as<unsigned long long>();
        A.ctl = d_ctl_.as<uint32_t>();
        A.prof = getenv("FISHRT_PERSIST_PROF") ? reinterpret_cast<unsigned long long*>(d_ctl_.as<uint32_t>() + 16) : nullptr;
        A.peer_stamps = (A.prof && d_sctl_.p) ? reinterpret_cast<const unsigned long long*>(d_sctl_.as<uint32_t>() + 16) + 16 : nullptr;
        set_naps(A.naps, "FISHRT_NAPS_FAST", persist_sampled_ ? kNapsFastSampled : kNapsFast);
        return A;
    }


    // ---- request rows (lm_persist_rows.hip): MFMA weight images, row edge buffers, per-row sampler / repetition-penalty state
    void ensure_rows(int R) {
        if constexpr (std::is_same<WT, bf16_t>::value || kFp8) {
            if (!d_rimg_.p) {
                d_rimg_.alloc(slow_persist_pack_bytes(a_.n_layer, false));  // (FS_FP8 too: the row images hold the e4m3 weights widened to bf16)
                d_rhimg_.alloc((size_t)PF_BLOCKS * PS_HEAD_IMAGE);
                if constexpr (kFp8) launch_rows_pack_fp8(slow_.data(), a_.n_layer, slow_head_w(), n_audio_, d_rimg_.p, d_rhimg_.p, st_);
                else launch_rows_pack(slow_.data(), a_.n_layer, slow_head_w(), n_audio_, d_rimg_.p, d_rhimg_.p, st_);
                if constexpr (!kFp8) {  // bf16 handles: the row kernels multiply every K-summed row result by a table entry unconditionally -- ones
                    const size_t n1 = (size_t)a_.n_layer * PF_BLOCKS * 48 + (size_t)PF_BLOCKS * 8 + (size_t)PF_BLOCKS * PF_SCL;
                    std::vector<float> ones(n1, 1.0f);
                    d_rones_.alloc(n1 * sizeof(float));
                    FS_HIP(hipMemcpyAsync(d_rones_.p, ones.data(), n1 * sizeof(float), hipMemcpyHostToDevice, st_));
                    FS_HIP(hipStreamSynchronize(st_));
                }
                d_rpairs_.alloc((size_t)PF_BLOCKS * 40 * PF_THREADS * 4);
                launch_rows_pack_rowpairs(d_pack_.p, d_rpairs_.p, st_);
                d_redges_s_.alloc(rows_slow_edge_bytes(PR_MAX_ROWS));
                FS_HIP(hipMemsetAsync(d_redges_s_.p, 0, d_redges_s_.n, st_));
                d_redges_f_.alloc(rows_fast_edge_bytes(PR_FAST_ROWS));
                FS_HIP(hipMemsetAsync(d_redges_f_.p, 0, d_redges_f_.n, st_));
                d_rctl_s_.alloc(256); d_rctl_f_.alloc(256);
                FS_HIP(hipMemsetAsync(d_rctl_s_.p, 0, 256, st_));
                FS_HIP(hipMemsetAsync(d_rctl_f_.p, 0, 256, st_));
                d_rlogits_.alloc(sizeof(float) * PR_MAX_ROWS * PR_LD);
                d_rcfg_.alloc(sizeof(SampleCfg) * PR_MAX_ROWS);
                d_rrng_.alloc(sizeof(RngState) * PR_MAX_ROWS);
                d_rbudget_.alloc(sizeof(int) * PR_MAX_ROWS);
                rrp_.alloc(PR_MAX_ROWS, a_.num_codebooks, a_.codebook_size);
                FS_HIP(hipStreamSynchronize(st_));
            }
            (void)R;
        } else {
            throw Error("request rows need a bf16 or fp8 handle");
        }
    }
    static constexpr int kNapsRowsSlow[6] = {28, 4, 8, 40, 24, 28}, kNapsRowsFast[6] = {20, 16, 16, 16, 20, 20};  // tools/tune_naps_rows.py at R = 4 (945 -> 933 us per frame; re-tuned after the half-block S2)
    RowsSlowArgs rows_slow_args(int R) {
        RowsSlowArgs A = {};
        A.wimg = d_rimg_.p; A.himg = d_rhimg_.p; A.norms = d_snorms_.as<float>();
        const float* sc0 = kFp8 ? d_sscl_.as<float>() : d_rones_.as<float>();  // FS_FP8: the slow persistent kernel's scale tables (same row -> workgroup mapping); bf16: ones
        A.scales = sc0;
        A.hscales = sc0 + (size_t)a_.n_layer * PF_BLOCKS * 48;
        A.n_layer = a_.n_layer; A.n_head_rows = n_audio_;
        A.cos_t = d_cos_.as<float>(); A.sin_t = d_sin_.as<float>(); A.eps = d_.eps;
        A.x = x(0); A.logits = d_rlogits_.as<float>(); A.state = state(0);
        A.kv_pool = kv_pool_.p; A.layer_half = (size_t)n_pages_ * page_elems_;
        A.page_table = d_page_table_.as<int>(); A.pt_stride = max_pages_;
        A.n_sl = std::max(1, std::min(nc_launch_, 16 / R));
        if (const char* c = getenv("FISHRT_ROWS_NSL_MAX")) A.n_sl = std::max(1, std::min(A.n_sl, atoi(c)));  // experiment: fewer, longer attention slices
        A.edges = d_redges_s_.as<unsigned long long>();
        A.ctl = d_rctl_s_.as<uint32_t>();
        A.prof = getenv("FISHRT_PERSIST_PROF") ? reinterpret_cast<unsigned long long*>(d_rctl_s_.as<uint32_t>() + 16) : nullptr;
        set_naps(A.naps, "FISHRT_NAPS_ROWS_SLOW", kNapsRowsSlow);
        return A;
    }
    RowsFastArgs rows_fast_args(int r0, int Rf) {
        RowsFastArgs A = {};
        (void)Rf;
        A.wpack = d_pack_.p; A.rowpairs = d_rpairs_.as<uint32_t>();
        A.scales = kFp8 ? d_fscl_.as<float>() : d_rones_.as<float>() + (size_t)a_.n_layer * PF_BLOCKS * 48 + (size_t)PF_BLOCKS * 8;
        for (int l = 0; l < PF_LAYERS; ++l) { A.norms[2 * l] = fast_[l].attn_norm; A.norms[2 * l + 1] = fast_[l].ffn_norm; }
        A.norms[2 * PF_LAYERS] = fast_norm_w_;
        A.fast_emb = fast_emb_; A.tok_emb = tok_emb_; A.cb_emb = cb_emb_;
        A.qkv0_tbl = (d_qkv0_.p && !getenv("FISHRT_ROWS_FAST_NO_QKV0")) ? d_qkv0_.as<float>() : nullptr;
        A.cos_t = d_cos_.as<float>(); A.sin_t = d_sin_.as<float>(); A.eps = d_.eps;
        A.xf = x(r0); A.x = x(r0);
        A.slow_logits = d_rlogits_.as<float>() + (size_t)r0 * PR_LD; A.n_slow = n_audio_;
        A.cap = cap_frames_ ? d_rcap_.as<float>() + (size_t)r0 * cap_frames_ * 9 * 2048 : nullptr; A.cap_frames = cap_frames_;
        A.state = state(r0); A.cfg = d_rcfg_.as<SampleCfg>() + r0; A.budget = d_rbudget_.as<int>() + r0; A.rng = d_rrng_.as<RngState>() + r0;
        const RepPenState rp = rrp_.view(r0);
        A.rp_mask = rp.mask; A.rp_ring = rp.ring; A.rp_meta = rp.ring_meta;
        A.out_codes = d_out_.as<uint32_t>() + (size_t)r0 * a_.num_codebooks * out_cap_; A.out_cap = out_cap_;
        A.edges = d_redges_f_.as<unsigned long long>();
        A.ctl = d_rctl_f_.as<uint32_t>();
        A.prof = getenv("FISHRT_PERSIST_PROF") ? reinterpret_cast<unsigned long long*>(d_rctl_f_.as<uint32_t>() + 16) : nullptr;
        set_naps(A.naps, "FISHRT_NAPS_ROWS_FAST", kNapsRowsFast);
        A.nap_draw = getenv("FISHRT_NAP_ROWS_DRAW") ? atoi(getenv("FISHRT_NAP_ROWS_DRAW")) : 16;  // flat between 0 and 48 (1075 us per sampled 4-row frame), 1088 at 96, 1111 at 200
        return A;
    }
    // the batch-1 fast kernel on row i of a multi-request call (FISHRT_ROWS_FAST_SINGLE: reference composition for the row fast kernel)
    FastPersistArgs persist_args(int i) {
        FastPersistArgs A = persist_args();
        A.xf = x(i); A.x = x(i);
        A.slow_logits = d_rlogits_.as<float>() + (size_t)i * PR_LD;
        A.cap = cap_frames_ ? d_rcap_.as<float>() + (size_t)i * cap_frames_ * 9 * 2048 : nullptr;
        A.state = state(i); A.cfg = d_rcfg_.as<SampleCfg>() + i; A.rp = rrp_.view(i); A.rng = d_rrng_.as<RngState>() + i;
        A.out_codes = d_out_.as<uint32_t>() + (size_t)i * a_.num_codebooks * out_cap_;
        return A;
    }

    // ---- kernel sequences
    void enqueue_slow_layers(int b) {
        for (int l = 0; l < a_.n_layer; ++l) {
            const LayerW& w = slow_[l];
            KVView kv = slow_kv(l, b);
            LmKernels<WT>::qkv(d_, x(b), w, d_cos_.as<float>(), d_sin_.as<float>(), state(b), 0, 0, d_q_.as<float>(), kv, st_);
            AttnKernels<WT>::decode(d_, d_q_.as<float>(), kv, state(b), d_part_.as<float>(), n_chunks_, nc_launch_, st_);
            LmKernels<WT>::wo(d_, d_part_.as<float>(), n_chunks_, nc_launch_, state(b), nullptr, kv, 0, w, x(b), st_);
            LmKernels<WT>::ffn_up(d_, x(b), w, d_act_.as<float>(), st_);
            LmKernels<WT>::ffn_down(d_, d_act_.as<float>(), w, x(b), st_);
        }
    }
    void enqueue_fast_layers(int b, int kv_pos, int rope_pos) {
        for (int l = 0; l < a_.n_fast_layer; ++l) {
            const LayerW& w = fast_[l];
            KVView kv = fast_kv(l, b);
            LmKernels<WT>::qkv(d_, xf(b), w, d_cos_.as<float>(), d_sin_.as<float>(), nullptr, kv_pos, rope_pos, d_q_.as<float>(), kv, st_);
            LmKernels<WT>::wo(d_, nullptr, 0, 0, nullptr, d_q_.as<float>(), kv, kv_pos + 1, w, xf(b), st_);
            LmKernels<WT>::ffn_up(d_, xf(b), w, d_act_.as<float>(), st_);
            LmKernels<WT>::ffn_down(d_, d_act_.as<float>(), w, xf(b), st_);
        }
    }

    // smallest power-of-two chunk count covering KV length T (the host knows every frame's position in advance)
    int chunk_bucket(int T) const {
        const int need = (T + AttnKernels<WT>::chunk() - 1) / AttnKernels<WT>::chunk();
        int b = 1;
        while (b < need) b <<= 1;
        return std::min(b, n_chunks_);
    }
    void set_bucket(int T) { nc_launch_ = chunk_bucket(T); }
    // graphs for the bucket currently in nc_launch_ (captured on first use)
    void use_graphs_for_bucket() {
        const int key = nc_launch_ * 8 + (use_persist_ && persist_sampled_ ? 4 : 0) + (use_persist_ ? 2 : 0) + (use_pslow_ ? 1 : 0);
        auto it = graphs_.find(key);
        if (it == graphs_.end()) {
            g_frame_ = nullptr; g_step_ = nullptr;
            build_graphs();
            graphs_[key] = {g_frame_, g_step_};
        } else {
            g_frame_ = it->second.first; g_step_ = it->second.second;
        }
    }
    void build_graphs() {
        if (g_frame_) return;
        FS_REQUIRE(a_.num_codebooks <= 8, "the fused fast-decoder attention holds at most 8 positions");
        const int C = a_.num_codebooks;
        hipGraph_t g = nullptr;
        // (1) prefill step: embed prompt column state->step, 24 blocks, pos++/step++
        FS_HIP(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
        LmKernels<WT>::embed(d_, tok_emb_, cb_emb_, C, a_.codebook_size, d_cfg_.as<SampleCfg>(), main_.prompt.as<uint32_t>(), state(0), x(0), st_);
        enqueue_slow_layers(0);
        launch_advance(state(0), st_);
        FS_HIP(hipStreamEndCapture(st_, &g));
        FS_HIP(hipGraphInstantiate(&g_step_, g, nullptr, nullptr, 0));
        FS_HIP(hipGraphDestroy(g));
        // (2) one audio frame: x holds the embedded input of position state->pos
        FS_HIP(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
        if (use_pslow_) launch_slow_persist(pslow_args(), st_);  // 24 blocks + head as ONE persistent launch (lm_persist_slow.hip)
        else {
        enqueue_slow_layers(0);
        // audio-range head: rows [im_end, V) only (constrain_probs_to_audio, utils.rs:13-16)
        LmKernels<WT>::head(d_, x(0), norm_w_, slow_head_w(), slow_head_s(), n_audio_, d_logits_slow_.as<float>(), st_);
        }
        if (!fold_slow_sampler())
            SampleKernels<WT>::sample_slow(d_, d_logits_slow_.as<float>(), n_audio_, d_cfg_.as<SampleCfg>(), d_rng_.as<RngState>(), state(0),
                                           x(0), xf(0), st_, d_hid_slot_.as<float*>());
        if (use_persist_) launch_fast_persist(persist_args(), persist_sampled_, st_);
        else
        for (int cbi = 0; cbi < C; ++cbi) {
            enqueue_fast_layers(0, cbi, cbi);
            LmKernels<WT>::head(d_, xf(0), fast_norm_w_, fast_out_w_, fast_out_s_, a_.codebook_size, d_logits_fast_.as<float>(), st_);
            SampleKernels<WT>::sample_fast(d_, d_logits_fast_.as<float>(), cbi, C, a_.codebook_size, d_cfg_.as<SampleCfg>(),
                                           d_rng_.as<RngState>(), rp_.view(0), state(0), fast_emb_, xf(0), tok_emb_, cb_emb_, x(0),
                                           d_out_.as<uint32_t>(), out_cap_, st_);
        }
        FS_HIP(hipStreamEndCapture(st_, &g));
        FS_HIP(hipGraphInstantiate(&g_frame_, g, nullptr, nullptr, 0));
        FS_HIP(hipGraphDestroy(g));
    }

    fs_model_args a_;
    fs_token_cfg t_;
    int device_, B_;
    ModelDims d_;
    int n_audio_ = 0;
    bool generic_ = false;  // DualAR token layout with <|im_end|> away from the semantic range (see the constructor)
    bool legacy_ = false;
    DevBuf d_legacy_head_;
    hipStream_t st_ = nullptr;
    bool loaded_ = false;
    // weights
    std::vector<TensorDesc> tensors_;
    size_t arena_bytes_ = 0, o_tok_emb_ = 0, o_cb_emb_ = 0, o_fast_emb_ = 0, o_norm_ = 0, o_fast_norm_ = 0;
    std::pair<size_t, size_t> o_out_ = {0, 0}, o_fast_out_ = {0, 0};
    std::vector<std::array<size_t, 10>> o_slow_, o_fast_;
    DevBuf arena_;
    std::vector<LayerW> slow_, fast_;
    const void *tok_emb_ = nullptr, *cb_emb_ = nullptr, *fast_emb_ = nullptr, *out_w_ = nullptr, *fast_out_w_ = nullptr;
    const float *norm_w_ = nullptr, *fast_norm_w_ = nullptr, *out_s_ = nullptr, *fast_out_s_ = nullptr;
    DevBuf d_cos_, d_sin_;
    // KV
    int max_pages_ = 0, n_pages_ = 0, out_cap_ = 0, n_chunks_ = 0, nc_launch_ = 1;
    std::map<int, std::pair<hipGraphExec_t, hipGraphExec_t>> graphs_;  // attention chunk bucket -> (frame, prefill-step) graphs
    std::map<int, hipGraphExec_t> multi_graphs_;                       // same key -> kFramesPerGraph frames of the two persistent launches in ONE graph
    // Measured with the launch-boundary stamps of FISHRT_PERSIST_PROF (s_memrealtime, one clock for all kernels): the slow kernel's finish ->
    // the fast kernel's entry inside a graph is 1.9 us, the fast kernel's finish -> the NEXT graph launch's slow kernel 7.2-7.3 us.  A graph
    // that holds several frames pays the 1.9 us edge between them (the kernels read positions / epochs from device memory, so a frame's two
    // launches are the same nodes every time; frames past <|im_end|> are no-ops on the device as in the per-frame replay).
    static int frames_per_graph() {
        static const int v = [] { const char* e = getenv("FISHRT_FRAMES_PER_GRAPH"); const int n = e ? atoi(e) : 8; return n < 0 ? 1 : (n > 32 ? 32 : n); }();  // 0: no graph, the two launches of every frame directly (experiment)
        return v;
    }
    hipGraphExec_t multi_frame_graph() {  // for the bucket currently in nc_launch_; the persistent 2-launch frame only
        const int key = nc_launch_ * 8 + (persist_sampled_ ? 4 : 0);
        auto it = multi_graphs_.find(key);
        if (it != multi_graphs_.end()) return it->second;
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        FS_HIP(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
        for (int f = 0; f < frames_per_graph(); ++f) {
            launch_slow_persist(pslow_args(), st_);
            launch_fast_persist(persist_args(), persist_sampled_, st_);
        }
        FS_HIP(hipStreamEndCapture(st_, &g));
        FS_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        FS_HIP(hipGraphDestroy(g));
        multi_graphs_[key] = ge;
        return ge;
    }
    size_t page_elems_ = 0;
    DevBuf kv_pool_, fast_pool_, d_page_table_, d_zero_table_;
    KvPages pages_;  // the slow KV pool's book: free list, reference counts, the sequences' and prefixes' page lists, the holds
    std::vector<int> seq_len_, fast_len_;
    // activations / state
    DevBuf d_x_, d_xf_, d_q_, d_part_, d_act_, d_logits_slow_, d_logits_fast_, d_state_, d_cfg_, d_rng_, d_out_;
    RepPenBufs rp_, srp_, rrp_;  // repetition-penalty state: the batch-1 generator's (1 row), the per-slot samplers' [max_batch] (allocated with d_scfg_), the request rows' [PR_MAX_ROWS] (ensure_rows)
    DevBuf d_pack_, d_edges_, d_ctl_, d_qkv0_;  // persistent fast decoder (+ the layer-0 qkv table of the codebook passes 1..7)
    DevBuf d_fscl_, d_sscl_;           // FS_FP8 handles: row scales of the persistent kernels' images
    DevBuf d_cap_;                     // fs_lm_debug_capture
    int cap_frames_ = 0;
    DevBuf d_hidden_, d_hid_slot_;     // generate_blocking_with_hidden: [out_cap][dim] rows + the pointer cell the captured graphs read
    bool persist_ok_ = false, use_persist_ = false, pslow_ok_ = false, use_pslow_ = false, persist_sampled_ = false;
    int batch_rows_ = 0, batch_row_ = 0;  // generate_batch_sequential: batch sampler semantics for the row being generated
    // continuous-batching session: per-slot remaining iterations (-1 = empty), host copy of the slot states, scratch KV page of empty slots
    bool sess_active_ = false;
    // what kind of session is open: set by session_begin together with sess_active_, {} again from session_end on (all false outside a session)
    struct SessMode {
        bool rows = false;     // FS_SESSION_ROWS (slots on the request-row kernels) ...
        bool sampled = false;  // ... whose slots all sample (else all greedy) ...
        int R = 0;             // ... and how many rows it has
        bool slots = false;    // FS_SESSION_PER_SLOT (slots on the static-batch step with the per-slot samplers)
        bool wide = false;     // FS_SESSION_WIDE_SAMPLER (the per-slot sampler nodes that also take nucleus-only / top_k > 256 settings)
        bool score = false;    // FS_SESSION_SCORE (the session's step graphs carry the 9 score nodes)
        bool trace = false;    // FS_SESSION_TRACE (... and the traced slots' tail node; the score nodes know the stash)
        int alts = 0;          // FS_SESSION_ALTS: N alternatives per decision (1 .. 16; the score nodes' second instantiation), 0 = off
    } sess_{};
    SampleCfg sess_cfg_ = {};  // the session's own SampleCfg (slots admitted without settings of their own)
    DevBuf d_scfg_, d_srng_;   // per-slot sampler state [max_batch] (k_sample_*_slots)
    int sess_adds_ = 0, sess_budget_tmp_ = 0;
    uint64_t sess_seed_ = 0;
    std::unique_lock<PersistLock> sess_plock_;
    std::vector<int> sess_left_, sess_pos_;
    std::vector<int> sess_L_;  // a live slot's total prompt length, prefix included (fs_lm_session_prefix_from_slot: T = L + frames - 1)
    std::vector<SeqState> sess_hs_;
    int sess_scratch_ = 0;  // (a hold of the page book's; a member because parked slots' rows are uploaded from here)
    uint64_t sess_released_frames_ = 0;
    std::vector<SessPrefix> sess_prefixes_;
    std::vector<SeqState> sess_stage_pos0_;            // a group pass's member start positions (pos; rope_off 0)
    std::vector<int> sess_stage_copy_;
    DevBuf d2_seqpos_, d2_copy_;                       // device copies of the two above: member start states / tail-copy page pairs
    DevBuf d_promo_pair_;                              // fs_lm_session_prefix_from_slot: the one (source, destination) page pair of its copy, read on the decode stream
    hipEvent_t ev_pft_[2] = {nullptr, nullptr};        // timing events around each prefill-stream pass (fs_lm_session_info)
    bool sess_timed_ = false;
    int64_t sess_count_[4] = {0, 0, 0, 0};             // passes, tokens prefilled, prefix tokens reused, tail pages copied
    double sess_pf_ms_ = 0.0;
    std::vector<uint32_t> sess_stage_prompts_;
    std::vector<int> sess_stage_rows_;
    std::vector<PendingAdd> sess_queue_, sess_flight_;  // joining requests: queued by session_admit / prefill launched (flush_pending)
    // prefix KV blobs: the handle's staging buffer (grow-only: the largest payload moved so far -- one export, or the imports of one pass),
    // the page ids of the prefixes being moved (device + the host vector the upload reads), the cached arena fingerprint
    DevBuf d_kvb_, d_kvb_pages_, d_fp_;
    std::vector<int> sess_stage_imp_pages_;
    bool fp_valid_ = false;
    uint64_t fp_ = 0;
    SlotTab<HidSlot> hid_;    // hidden-state collectors (fs_lm_session_add_hidden): the table of the step's k_hidden_rows node
    SlotTab<ScoreSlot> sc_;   // scoring slots (fs_lm_session_add_scored): the table of the step's k_score_slots nodes
    std::vector<char> sess_traced_;  // per slot: admitted with fs_lm_session_add_traced (its sc_ entry has no targets)
    DevBuf d_trace_;                 // the traced slots' stash f32 [B][TRACE_STASH_WORDS] (lm_kernels.h), once per handle
    SeqState sess_stage_ = {};
    hipStream_t st_pf_ = nullptr;
    hipEvent_t ev_pf_ = nullptr;
    PrefillLane join_{st_pf_};  // row buffers and staged prompt of the session's prefill stream
    DevBuf d_spack_, d_hpack_, d_snorms_, d_sedges_, d_sctl_;  // persistent slow transformer
    PrefillLane main_{st_};  // MFMA row-path activations (kRowsCap rows) of the engine stream: prefill passes and the static-batch steps; the one staged prompt
    DevBuf d_bprompt_;  // static batch: all left-padded prompts [B][C + 1][Lmax] (group prefill)
    DevBuf d_xfrows_, d_lrows_, d_lfast_, d_fast_state_, d_fast_table_, d_rwords_;  // static-batch generator
    DevBuf d_xchg_, d_epoch_;  // folded decode steps: split-K exchange units, {step epoch, timeouts}
    bool rows_par_ = false;  // this batch / session samples with the block-parallel row samplers
    int ld_slow_ = 0, down_split_ = 4;
    bool fold_off_ = false;  // set after a reported exchange timeout of the folded decode step: the handle keeps the slab path from then on
    std::map<long long, hipGraphExec_t> batch_graphs_;
    DevBuf d_rimg_, d_rhimg_, d_redges_s_, d_redges_f_, d_rctl_s_, d_rctl_f_, d_rlogits_, d_rcfg_, d_rrng_, d_rbudget_;  // request rows (lm_persist_rows.hip)
    DevBuf d_rcap_, d_rpairs_, d_rones_;
    void* h_pin_ = nullptr;
    hipGraphExec_t g_frame_ = nullptr, g_step_ = nullptr;
    hipEvent_t ev_[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_batch_[2] = {nullptr, nullptr};  // decode batches in flight (generate)
    fs_gen_stats stats_ = {};
};

void fp8_quantize_rows(int device, const float* w, int64_t rows, int64_t cols, uint8_t* q_out, float* scales_out) {
    FS_REQUIRE(rows >= 1 && cols >= 1 && rows < (1ll << 31), "bad matrix shape");
    FS_HIP(hipSetDevice(device));
    DevBuf src, q, sc;
    src.alloc((size_t)rows * cols * 4); q.alloc((size_t)rows * cols); sc.alloc((size_t)rows * 4);
    FS_HIP(hipMemcpy(src.p, w, (size_t)rows * cols * 4, hipMemcpyHostToDevice));
    launch_quant_rows_fp8(q.as<uint8_t>(), sc.as<float>(), src.as<float>(), rows, cols, 1, 0, nullptr);
    FS_HIP(hipDeviceSynchronize());
    FS_HIP(hipMemcpy(q_out, q.p, (size_t)rows * cols, hipMemcpyDeviceToHost));
    FS_HIP(hipMemcpy(scales_out, sc.p, (size_t)rows * 4, hipMemcpyDeviceToHost));
}
void fp8_decode_table(int device, float* out) {
    FS_HIP(hipSetDevice(device));
    DevBuf t;
    t.alloc(16 * 256 * 4);
    launch_fp8_decode_table(t.as<float>(), nullptr);
    FS_HIP(hipDeviceSynchronize());
    FS_HIP(hipMemcpy(out, t.p, 16 * 256 * 4, hipMemcpyDeviceToHost));
}

LMBase* make_lm(const fs_model_args& a, const fs_token_cfg& t, int device, fs_dtype dtype, int max_batch) {
    if (dtype == FS_BF16) return new LM<bf16_t>(a, t, device, max_batch);
    if (dtype == FS_F32) return new LM<float>(a, t, device, max_batch);
    if (dtype == FS_FP8) return new LM<fp8_t>(a, t, device, max_batch);
    throw Error("unknown dtype");
}

}  // namespace fs
