// m3_api.hip -- the C ABI of include/m3.h (kernels and launchers: m3_kernels.hpp).
#include "m3_kernels.hpp"
#include "m3_search.hpp"
#include "m3_net.hpp"
#include "m3_search_nn.hpp"

#include <string>

namespace {
thread_local std::string g_err;
}  // namespace

int set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#ifdef M3_SPLIT_TU  // the launchers are instantiated in m3_inst.hip, one TU per configuration
namespace m3k {
M3_INSTANTIATE(extern template, CF_0)
M3_INSTANTIATE(extern template, CF_1)
#ifndef M3_HEADLINE_ONLY  // A/B builds of the two specialised shapes only (Makefile `variant-fast`)
M3_INSTANTIATE(extern template, CF_2)
M3_INSTANTIATE(extern template, CF_3)
M3_INSTANTIATE(extern template, CF_4)
M3_INSTANTIATE(extern template, CF_5)
#ifndef M3_NO_WIDE_FRAME  // (Makefile `variant-frame16`: no 32 x 32 frame)
M3_INSTANTIATE(extern template, CF_6)
M3_INSTANTIATE(extern template, CF_7)
M3_INSTANTIATE(extern template, CF_8)
M3_INSTANTIATE(extern template, CF_9)
#endif
#endif
}  // namespace m3k
#endif
using namespace m3k;

namespace {
// rows < columns: the last action ids decode to a swap with the row below the
// board, and the reference's legal_actions / apply_action raise IndexError on
// every call (boardConfig.py:27,45-59; boardv2.py:188 calls legal_actions in
// every step). Such a BoardConfig resets (BoardV2.__init__) but cannot step.
int check_ids_on_board(const m3_ctx* c) {
    if (c->R >= c->C) return M3_OK;
    return set_err(M3_ERR_INVALID,
                   "BoardConfig(rows=%d, columns=%d): action ids reach row %d, past the board; the reference's "
                   "legal_actions / apply_action raise IndexError for rows < columns", c->R, c->C, c->R);
}

int ensure_scratch(m3_ctx* c, size_t bytes) {
    if (c->dcap >= bytes) return M3_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));  // async work may still use the old buffer
    if (c->dbuf) HIP_TRY(hipFree(c->dbuf));
    c->dbuf = nullptr;
    c->dcap = 0;
    HIP_TRY(hipMalloc(&c->dbuf, bytes));
    c->dcap = bytes;
    return M3_OK;
}

int ensure_host(m3_ctx* c, size_t bytes) {
    if (c->hcap >= bytes) return M3_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->hbuf) HIP_TRY(hipHostFree(c->hbuf));
    c->hbuf = nullptr;
    c->hdev = nullptr;
    c->hcap = 0;
    HIP_TRY(hipHostMalloc(&c->hbuf, bytes, hipHostMallocMapped | hipHostMallocPortable));
    HIP_TRY(hipHostGetDevicePointer(&c->hdev, c->hbuf, 0));  // the device's address of the same bytes
    c->hcap = bytes;
    return M3_OK;
}

constexpr size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// Small host-buffer calls (the facade's batch-1 calls) run zero-copy; m3_rollouts is staged at every n.
constexpr int64_t ZC_MAX_BOARDS = 256;
constexpr int ZC_OVF_WORD = 8;  // c->counters[8]: the zero-copy overflow count, kept zero between calls

// One host-buffer call. The call registers its parts once (input / output, each 256-byte aligned),
// then begin() -> fill the kernel arguments from dev() / lead_dev() / tail() -> launch -> finish().
//   staged:    the inputs are packed into the context's pinned buffer and go up in ONE copy, which
//              also zeroes the `lead` bytes in front of the outputs (the launch's counters); the
//              outputs come back in ONE copy and are unpacked: two copies, the launches and a sync,
//              instead of a pageable copy per array. Device scratch = [input image | output image
//              | device-only tail]; the pinned buffer holds the larger of the two images.
//   zero-copy: the kernels read the inputs from and write the outputs to the pinned buffer itself
//              (host memory the device maps, one combined image), so a call is its launches and
//              one sync, with no copy in either direction. The tail is the device scratch.
class HostCall {
public:
    explicit HostCall(m3_ctx* c) : c_(c) {}
    int input(const void* src, size_t bytes) { return add({bytes, src, nullptr, 0}, in_total_); }
    // dst == nullptr: the caller does not want it (no bytes; its device address is nullptr)
    int output(void* dst, size_t bytes) { return add({dst ? bytes : 0, nullptr, dst, 0}, out_total_); }

    // lead: bytes in front of the outputs that are zero before the launch; tail: device-only bytes
    int begin(bool zc, size_t lead, size_t tail) {
        if (n_ > MAXP) return set_err(M3_ERR_INVALID, "internal: a host-buffer call with more than %d parts", MAXP);
        zc_ = zc;
        for (int i = 0; i < n_; ++i)
            if (!parts_[i].src) parts_[i].off += align256(lead);  // the outputs follow the lead bytes
        out_total_ += align256(lead);
        const size_t in_sz = align256(in_total_), out_sz = align256(out_total_);
        int rc = ensure_host(c_, (zc ? in_sz + out_total_ : std::max(in_sz, out_sz)) + 256);
        const size_t scratch = zc ? tail : in_sz + out_sz + tail;
        if (rc == M3_OK && scratch) rc = ensure_scratch(c_, scratch + 256);
        if (rc) return rc;
        char* h = (char*)c_->hbuf;  // (hbuf / hdev / dbuf are read only after they have grown)
        din_ = (char*)(zc ? c_->hdev : c_->dbuf);
        dout_ = din_ + in_sz;
        hout_ = zc ? h + in_sz : h;
        tail_ = zc ? (char*)c_->dbuf : dout_ + out_sz;
        for (int i = 0; i < n_; ++i)
            if (parts_[i].src) memcpy(h + parts_[i].off, parts_[i].src, parts_[i].bytes);
        if (zc) {
            memset(hout_, 0, lead);
            return M3_OK;
        }
        memset(h + in_total_, 0, in_sz + lead - in_total_);
        HIP_TRY(hipMemcpyAsync(din_, h, in_sz + lead, hipMemcpyHostToDevice, c_->stream));
        return M3_OK;
    }

    template <class T>
    T* dev(int part) const {
        const Part& p = parts_[part];
        return p.bytes ? reinterpret_cast<T*>((p.src ? din_ : dout_) + p.off) : nullptr;
    }
    uint32_t* lead_dev() const { return reinterpret_cast<uint32_t*>(dout_); }
    const uint32_t* lead_host() const { return reinterpret_cast<const uint32_t*>(hout_); }  // after finish()
    char* tail() const { return tail_; }

    // wait for the launches (staged: behind the one download) and unpack the outputs
    int finish() {
        if (!zc_) HIP_TRY(hipMemcpyAsync(hout_, dout_, out_total_, hipMemcpyDeviceToHost, c_->stream));
        HIP_TRY(hipStreamSynchronize(c_->stream));
        for (int i = 0; i < n_; ++i)
            if (parts_[i].dst) memcpy(parts_[i].dst, hout_ + parts_[i].off, parts_[i].bytes);
        return M3_OK;
    }

private:
    struct Part {
        size_t bytes;
        const void* src;  // input: the caller's buffer
        void* dst;        // output: the caller's buffer
        size_t off;       // in its image
    };
    // (a fixed array: no heap allocation per call. A part too many is only counted: begin() refuses the call.)
    int add(Part p, size_t& total) {
        if (n_ < MAXP) {
            p.off = total = align256(total);
            total += p.bytes;
            parts_[n_] = p;
        }
        return n_++;
    }
    static constexpr int MAXP = 12;
    m3_ctx* c_;
    Part parts_[MAXP];
    int n_ = 0;
    size_t in_total_ = 0, out_total_ = 0;
    bool zc_ = false;
    char *din_ = nullptr, *dout_ = nullptr, *hout_ = nullptr, *tail_ = nullptr;
};

int bad_cells_error() {
    return set_err(M3_ERR_INVALID, "cell value outside [0, 127] in the boards (outputs undefined)");
}

int not_ready_error(const char* entry) {
    return set_err(M3_ERR_STATE, "%s before m3_env_reset (or before m3_env_set of boards, seeds, score, moves and "
                                 "next_action)", entry);
}

// Make `st` wait for every shard's last enqueued work.
int join_shards(m3_env* e, hipStream_t st) {
    for (auto& sh : e->shards)
        if (sh.n) HIP_TRY(hipStreamWaitEvent(st, sh.ev, 0));
    return M3_OK;
}

int sync_env(m3_env* e) {
    for (auto& sh : e->shards) {
        HIP_TRY(hipStreamSynchronize(sh.stream));
        HIP_TRY(hipStreamSynchronize(sh.pstream));
        for (bool& p : sh.ppending) p = false;
        for (bool& p : sh.apending) p = false;
    }
    if (e->ustream) HIP_TRY(hipStreamSynchronize(e->ustream));
    e->upload_pend[0] = e->upload_pend[1] = false;
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    return M3_OK;
}

void destroy_shards(m3_env* e) {
    for (auto& sh : e->shards) {
        (void)hipStreamDestroy(sh.stream);
        (void)hipStreamDestroy(sh.pstream);
        (void)hipEventDestroy(sh.ev);
        for (hipEvent_t ev : sh.pev) (void)hipEventDestroy(ev);
        for (hipEvent_t ev : sh.aev) (void)hipEventDestroy(ev);
    }
    e->shards.clear();
}

// A device buffer of the env: allocated into *field, recorded in e->owned (m3_env_destroy frees it),
// and with `zero` filled with zeros on the context stream (the caller synchronises it).
template <class T>
hipError_t env_alloc(m3_env* e, T** field, size_t bytes, bool zero) {
    hipError_t err = hipMalloc((void**)field, bytes ? bytes : 4);
    if (err != hipSuccess) return err;
    e->owned.push_back(*field);
    return zero ? hipMemsetAsync(*field, 0, bytes, e->ctx->stream) : hipSuccess;
}
}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
// configuration id (shape_id) -> its config type (CF_<id>, m3_kernels.hpp)
template <class F>
static int with_shape(int shape, F&& f) {
    static_assert(N_CONFIGS == 10, "with_shape lists every configuration");
    switch (shape) {
        case 0: return f(CF_0{});
        case 1: return f(CF_1{});
#ifndef M3_HEADLINE_ONLY
        case 2: return f(CF_2{});
        case 3: return f(CF_3{});
        case 4: return f(CF_4{});
        case 5: return f(CF_5{});
#ifndef M3_NO_WIDE_FRAME
        case 6: return f(CF_6{});
        case 7: return f(CF_7{});
        case 8: return f(CF_8{});
        case 9: return f(CF_9{});
#endif
#endif
        default: return set_err(M3_ERR_UNSUPPORTED, "board shape not compiled in");
    }
}

static int ensure_fresh(m3_env* e) {
    if (!e->stale) return M3_OK;
    return with_shape(e->ctx->shape, [&](auto cf) { return rederive<decltype(cf)>(e); });
}

extern "C" {

int m3_abi_version(void) { return M3_ABI_VERSION; }

const char* m3_last_error(void) { return g_err.c_str(); }

int m3_device_count(int* out) {
    CHECK_ARG(out, "null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *out = (e == hipSuccess) ? n : 0;
    return M3_OK;
}

int m3_supported(int rows, int columns, int types) { return shape_id(rows, columns, types) >= 0 ? 1 : 0; }

int m3_action_space(int rows, int columns, int* out_actions, int* out_words) {
    CHECK_ARG(rows > 0 && columns > 0, "bad shape");
    const int A = rows * (columns - 1) * 2;
    if (out_actions) *out_actions = A;
    if (out_words) *out_words = (A + 31) / 32;
    return M3_OK;
}

int m3_ctx_create(int device, int rows, int columns, int types, m3_ctx** out) {
    CHECK_ARG(out, "null out");
    *out = nullptr;
    const int sid = shape_id(rows, columns, types);
    if (sid < 0)
        return set_err(M3_ERR_UNSUPPORTED,
                       "BoardConfig(rows=%d, columns=%d, types=%d): supported are rows and columns 3..32, "
                       "types 2..31", rows, columns, types);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return set_err(M3_ERR_NO_DEVICE, "no HIP device visible (libm3 has no CPU fallback)");
    CHECK_ARG(device >= 0 && device < ndev, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(M3_ERR_NO_DEVICE, "device %d is %s; libm3 is built for gfx950 only", device, prop.gcnArchName);
    m3_ctx* c = new m3_ctx;
    c->device = device;
    c->R = rows;
    c->C = columns;
    c->T = types;
    c->N = rows * columns;
    c->A = rows * (columns - 1) * 2;
    c->AW = (c->A + 31) / 32;
    c->shape = sid;
    c->sdesc = make_shape(rows, columns, types);
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&c->counters, 256);
    // (the zero-copy overflow word starts at zero.) On the context's own stream, and finished before
    // the context is handed out: hipMemset runs on the null stream and may return before the fill is
    // done, and the context stream is non-blocking, so it does not wait for the null stream
    if (e == hipSuccess) e = hipMemsetAsync(c->counters, 0, 256, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        delete c;
        return set_err(M3_ERR_HIP, "context setup: %s", hipGetErrorString(e));
    }
    *out = c;
    return M3_OK;
}

int m3_ctx_destroy(m3_ctx* c) {
    if (!c) return M3_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->dbuf) (void)hipFree(c->dbuf);
    if (c->hbuf) (void)hipHostFree(c->hbuf);
    if (c->counters) (void)hipFree(c->counters);
    for (hipEvent_t ev : c->tev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return M3_OK;
}

int m3_ctx_synchronize(m3_ctx* c) {
    CHECK_ARG(c, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return M3_OK;
}

int m3_dev_alloc(m3_ctx* c, int64_t bytes, void** out) {
    CHECK_ARG(c && out && bytes >= 0, "bad arguments");
    *out = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(out, bytes ? (size_t)bytes : 4));
    return M3_OK;
}

int m3_dev_free(m3_ctx* c, void* p) {
    CHECK_ARG(c, "null ctx");
    if (!p) return M3_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));  // the context's work may still use it
    HIP_TRY(hipFree(p));
    return M3_OK;
}

int m3_dev_copy(m3_ctx* c, void* dst, const void* src, int64_t bytes, int kind) {
    CHECK_ARG(c && dst && src && bytes >= 0 && (kind == 1 || kind == 2), "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return M3_OK;
}

int m3_init_boards_ex(m3_ctx* c, int64_t n, const uint32_t* seeds, int8_t* out_boards, uint32_t* out_draws,
                      int32_t* out_first_action, uint32_t* out_flags) {
    CHECK_ARG(c && n >= 0 && (n == 0 || (seeds && out_boards)), "bad arguments");
    if (n == 0) return M3_OK;
    HIP_TRY(hipSetDevice(c->device));
    HostCall hc(c);
    const int i_s = hc.input(seeds, n * 4ull);
    const int o_b = hc.output(out_boards, n * (size_t)c->N), o_d = hc.output(out_draws, n * 4ull),
              o_f = hc.output(out_first_action, n * 4ull), o_g = hc.output(out_flags, n * 4ull);
    int rc = hc.begin(n <= ZC_MAX_BOARDS, 0, 0);
    if (rc) return rc;
    InitArgs a{};
    a.shape = c->sdesc;
    a.n = n;
    a.seeds = hc.dev<const uint32_t>(i_s);
    a.boards = hc.dev<int8_t>(o_b);
    a.draws = hc.dev<uint32_t>(o_d);
    a.first_action = hc.dev<int32_t>(o_f);
    a.flags = hc.dev<uint32_t>(o_g);
    rc = with_shape(c->shape, [&](auto cf) { return launch_init<decltype(cf)>(c->stream, a, n); });
    if (rc) return rc;
    return hc.finish();
}

int m3_init_boards(m3_ctx* c, int64_t n, const uint32_t* seeds, int8_t* out_boards, uint32_t* out_draws,
                   int32_t* out_first_action) {
    std::vector<uint32_t> flags(n > 0 ? (size_t)n : 0);
    int rc = m3_init_boards_ex(c, n, seeds, out_boards, out_draws, out_first_action, flags.data());
    if (rc) return rc;
    int64_t capped = 0;
    for (uint32_t f : flags) capped += (f & M3_FLAG_RESET_CAP) != 0;
    if (capped)  // the reference keeps drawing (boardv2.py:23-27): no result to return
        return set_err(M3_ERR_CAP, "%lld of %lld resets stopped at the redraw-round cap (M3_FLAG_RESET_CAP; "
                       "m3_init_boards_ex returns the flags per board)", (long long)capped, (long long)n);
    return M3_OK;
}

int m3_apply_actions(m3_ctx* c, int64_t n, const int8_t* boards, const uint32_t* seeds, const int32_t* n_actions,
                     const int32_t* actions, int8_t* out_boards, int32_t* out_reward, uint32_t* out_draws,
                     uint32_t* out_flags, uint32_t* out_legal_bits, int32_t* out_next_action) {
    CHECK_ARG(c && n >= 0, "bad arguments");
    if (n == 0) return M3_OK;
    CHECK_ARG(boards && seeds && n_actions && actions && out_boards && out_reward && out_draws && out_flags,
              "null buffer");
    int rc = check_ids_on_board(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = n * (size_t)c->N;
    const bool zc = n <= ZC_MAX_BOARDS;
    HostCall hc(c);  // cell values are checked on the device while the boards are staged (k_apply)
    const int i_b = hc.input(boards, bytes), i_s = hc.input(seeds, n * 4ull), i_na = hc.input(n_actions, n * 4ull),
              i_a = hc.input(actions, n * 4ull);
    const int o_b = hc.output(out_boards, bytes), o_r = hc.output(out_reward, n * 4ull),
              o_d = hc.output(out_draws, n * 4ull), o_f = hc.output(out_flags, n * 4ull),
              o_l = hc.output(out_legal_bits, n * 4ull * c->AW), o_x = hc.output(out_next_action, n * 4ull);
    rc = hc.begin(zc, 16, n * 4ull);  // lead words: [0] overflow count (staged), [1] bad cells; tail: overflow list
    if (rc) return rc;
    ApplyArgs a{};
    a.shape = c->sdesc;
    a.n = n;
    a.boards = hc.dev<const int8_t>(i_b);
    a.seeds = hc.dev<const uint32_t>(i_s);
    a.n_actions = hc.dev<const int32_t>(i_na);
    a.actions = hc.dev<const int32_t>(i_a);
    a.out_boards = hc.dev<int8_t>(o_b);
    a.reward = hc.dev<int32_t>(o_r);
    a.draws = hc.dev<uint32_t>(o_d);
    a.flags = hc.dev<uint32_t>(o_f);
    a.legal = hc.dev<uint32_t>(o_l);
    a.next_action = hc.dev<int32_t>(o_x);
    // zero-copy: the count is a device word that k_apply_fix, launched with one block, clears again;
    // staged: lead word 0, zeroed by the upload
    a.ovf_count = zc ? c->counters + ZC_OVF_WORD : hc.lead_dev();
    a.clear_ovf = zc ? 1 : 0;
    a.bad_cells = hc.lead_dev() + 1;
    a.ovf_list = (uint32_t*)hc.tail();
    rc = with_shape(c->shape, [&](auto cf) { return launch_apply<decltype(cf)>(c, a); });
    if (rc) {
        if (zc) {  // k_apply may have counted overflows that k_apply_fix never cleared: the next
                   // call must not read them (best effort; the launch error is what is reported)
            (void)hipMemsetAsync(a.ovf_count, 0, 4, c->stream);  // (ordered before the next call's kernels)
            (void)hipStreamSynchronize(c->stream);
        }
        return rc;
    }
    rc = hc.finish();
    if (rc) return rc;
    return hc.lead_host()[1] ? bad_cells_error() : M3_OK;
}

int m3_legal_actions(m3_ctx* c, int64_t n, const int8_t* boards, uint32_t* out_legal_bits) {
    CHECK_ARG(c && n >= 0, "bad arguments");
    if (n == 0) return M3_OK;
    CHECK_ARG(boards && out_legal_bits, "null buffer");
    int rc = check_ids_on_board(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HostCall hc(c);
    const int i_b = hc.input(boards, n * (size_t)c->N), o_l = hc.output(out_legal_bits, n * 4ull * c->AW);
    rc = hc.begin(n <= ZC_MAX_BOARDS, 0, 0);
    if (rc) return rc;
    rc = with_shape(c->shape, [&](auto cf) {
        return launch_legal<decltype(cf)>(c, n, hc.dev<const int8_t>(i_b), hc.dev<uint32_t>(o_l));
    });
    if (rc) return rc;
    return hc.finish();
}

// ---- one-ply lookahead --------------------------------------------------------
constexpr int LOOK_OVF_WORD = 12;  // c->counters[12]: the lookahead's exact-pass count (zeroed per call)

// The checks that the host-buffer and the device-buffer form of a batch call share; the caller
// returns at once if this fails or n == 0. `buffers`: every required pointer is non-null.
static int batch_call_preamble(m3_ctx* c, int64_t n, bool buffers) {
    CHECK_ARG(c && n >= 0, "bad arguments");
    if (n == 0) return M3_OK;
    CHECK_ARG(n < (int64_t)1 << 31, "n too large");
    CHECK_ARG(buffers, "null buffer");
    int rc = check_ids_on_board(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return M3_OK;
}

// a.n, the inputs and the outputs set; the exact pass's list comes from `list` ([n] words of device memory)
static int enqueue_lookahead(m3_ctx* c, LookArgs a, uint32_t* list) {
    a.shape = c->sdesc;
    a.ovf_count = c->counters + LOOK_OVF_WORD;
    a.ovf_list = list;
    HIP_TRY(hipMemsetAsync(a.ovf_count, 0, 4, c->stream));
    return with_shape(c->shape, [&](auto cf) { return launch_lookahead<decltype(cf)>(c->stream, a); });
}

int m3_lookahead_device(m3_ctx* c, int64_t n, const int8_t* boards, const uint32_t* seeds, const int32_t* n_actions,
                        int32_t* out_best_action, int32_t* out_best_reward, int32_t* out_values,
                        uint32_t* out_last_draws, uint32_t* out_flags) {
    int rc = batch_call_preamble(c, n, boards && seeds && n_actions);
    if (rc || n == 0) return rc;
    rc = ensure_scratch(c, n * 4ull + 256);
    if (rc) return rc;
    LookArgs a{};
    a.n = n;
    a.boards = boards;
    a.seeds = seeds;
    a.n_actions = n_actions;
    a.best_action = out_best_action;
    a.best_reward = out_best_reward;
    a.values = out_values;
    a.last_draws = out_last_draws;
    a.flags = out_flags;
    return enqueue_lookahead(c, a, (uint32_t*)c->dbuf);
}

int m3_lookahead(m3_ctx* c, int64_t n, const int8_t* boards, const uint32_t* seeds, const int32_t* n_actions,
                 int32_t* out_best_action, int32_t* out_best_reward, int32_t* out_values, uint32_t* out_last_draws,
                 uint32_t* out_flags) {
    int rc = batch_call_preamble(c, n, boards && seeds && n_actions);
    if (rc || n == 0) return rc;
    HostCall hc(c);
    const int i_b = hc.input(boards, n * (size_t)c->N), i_s = hc.input(seeds, n * 4ull),
              i_na = hc.input(n_actions, n * 4ull);
    const int o_a = hc.output(out_best_action, n * 4ull), o_r = hc.output(out_best_reward, n * 4ull),
              o_v = hc.output(out_values, n * 4ull * c->A), o_d = hc.output(out_last_draws, n * 4ull),
              o_f = hc.output(out_flags, n * 4ull);
    rc = hc.begin(n <= ZC_MAX_BOARDS, 16, n * 4ull);  // lead word [0]: bad cells; tail: the exact pass's list
    if (rc) return rc;
    LookArgs a{};
    a.n = n;
    a.boards = hc.dev<const int8_t>(i_b);
    a.seeds = hc.dev<const uint32_t>(i_s);
    a.n_actions = hc.dev<const int32_t>(i_na);
    a.bad_cells = hc.lead_dev();
    a.best_action = hc.dev<int32_t>(o_a);
    a.best_reward = hc.dev<int32_t>(o_r);
    a.values = hc.dev<int32_t>(o_v);
    a.last_draws = hc.dev<uint32_t>(o_d);
    a.flags = hc.dev<uint32_t>(o_f);
    rc = enqueue_lookahead(c, a, (uint32_t*)hc.tail());
    if (rc) return rc;
    rc = hc.finish();
    if (rc) return rc;
    return hc.lead_host()[0] ? bad_cells_error() : M3_OK;
}

// ---- rollouts ---------------------------------------------------------------
}  // extern "C"

namespace {

size_t rollout_spill_words(int shape) {
    return (size_t)with_shape(shape, [&](auto cf) {
        using CF = decltype(cf);
        return (int)LdsStore<CF, KS<CF>::GCAP, KS<CF>::B>::SPILL_WORDS;
    });
}

// device-only bytes of a rollout launch: [overflow list, n words | spill pool], each 256-byte aligned
size_t rollout_pool_bytes(int shape, int64_t n) {
    return rollout_spill_cap(n, rollout_spill_words(shape)) * rollout_spill_words(shape) * 4ull;
}
size_t rollout_tail_bytes(int shape, int64_t n) { return align256(n * 4ull) + rollout_pool_bytes(shape, n) + 256; }

// a.n and the per-rollout buffers set; `tail`: rollout_tail_bytes of device memory, 256-byte aligned.
// counters: 16 zeroed bytes on the device (nullptr: the context's, zeroed here)
int enqueue_rollouts(m3_ctx* c, RolloutArgs a, char* tail, uint32_t* counters = nullptr) {
    if (!counters) {
        counters = c->counters;
        HIP_TRY(hipMemsetAsync(counters, 0, 16, c->stream));
    }
    a.shape = c->sdesc;
    a.counters = counters;
    a.ovf_list = (uint32_t*)tail;
    a.spill = (uint32_t*)(tail + align256(a.n * 4ull));
    a.spill_cap = (uint32_t)rollout_spill_cap(a.n, rollout_spill_words(c->shape));
    return with_shape(c->shape, [&](auto cf) { return launch_rollouts<decltype(cf)>(c, a); });
}

}  // namespace

extern "C" {

int m3_rollouts_device(m3_ctx* c, int64_t n, const int8_t* boards, const uint32_t* seeds, const int32_t* n_actions,
                       const uint32_t* rollout_seeds, int32_t* out_gain, int32_t* out_steps, uint32_t* out_draws,
                       uint32_t* out_flags, int8_t* out_boards) {
    int rc = batch_call_preamble(c, n, boards && seeds && n_actions && rollout_seeds && out_gain && out_steps &&
                                           out_draws && out_flags);
    if (rc || n == 0) return rc;
    rc = ensure_scratch(c, rollout_tail_bytes(c->shape, n));
    if (rc) return rc;
    RolloutArgs a{};
    a.n = n;
    a.boards = boards;
    a.seeds = seeds;
    a.n_actions = n_actions;
    a.rseeds = rollout_seeds;
    a.gain = out_gain;
    a.steps = out_steps;
    a.draws = out_draws;
    a.flags = out_flags;
    a.out_boards = out_boards;
    return enqueue_rollouts(c, a, (char*)c->dbuf);
}

int m3_rollouts(m3_ctx* c, int64_t n, const int8_t* boards, const uint32_t* seeds, const int32_t* n_actions,
                const uint32_t* rollout_seeds, int32_t* out_gain, int32_t* out_steps, uint32_t* out_draws,
                uint32_t* out_flags, int8_t* out_boards) {
    int rc = batch_call_preamble(c, n, boards && seeds && n_actions && rollout_seeds && out_gain && out_steps &&
                                           out_draws && out_flags);
    if (rc || n == 0) return rc;
    const size_t bytes = n * (size_t)c->N;
    HostCall hc(c);  // cell values are checked on the device while the boards are staged (k_rollout)
    const int i_b = hc.input(boards, bytes), i_s = hc.input(seeds, n * 4ull), i_na = hc.input(n_actions, n * 4ull),
              i_rs = hc.input(rollout_seeds, n * 4ull);
    const int o_g = hc.output(out_gain, n * 4ull), o_st = hc.output(out_steps, n * 4ull),
              o_d = hc.output(out_draws, n * 4ull), o_f = hc.output(out_flags, n * 4ull),
              o_b = hc.output(out_boards, bytes);
    rc = hc.begin(false, 16, rollout_tail_bytes(c->shape, n));  // staged at every n; lead: the launch's counters
    if (rc) return rc;
    RolloutArgs a{};
    a.n = n;
    a.boards = hc.dev<const int8_t>(i_b);
    a.seeds = hc.dev<const uint32_t>(i_s);
    a.n_actions = hc.dev<const int32_t>(i_na);
    a.rseeds = hc.dev<const uint32_t>(i_rs);
    a.gain = hc.dev<int32_t>(o_g);
    a.steps = hc.dev<int32_t>(o_st);
    a.draws = hc.dev<uint32_t>(o_d);
    a.flags = hc.dev<uint32_t>(o_f);
    a.out_boards = hc.dev<int8_t>(o_b);
    rc = enqueue_rollouts(c, a, hc.tail(), hc.lead_dev());
    if (rc) return rc;
    rc = hc.finish();
    if (rc) return rc;
    return hc.lead_host()[2] ? bad_cells_error() : M3_OK;
}

// ---- env ------------------------------------------------------------------
int m3_env_create(m3_ctx* c, int64_t n, int num_moves, int env_goal, m3_env** out) {
    CHECK_ARG(c && out && n > 0 && num_moves > 0, "bad arguments");
    CHECK_ARG(n < (int64_t)1 << 31, "n too large");
    int rc0 = check_ids_on_board(c);
    if (rc0) return rc0;
    *out = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    m3_env* e = new m3_env;
    e->ctx = c;
    e->n = n;
    e->num_moves = num_moves;
    e->goal = env_goal;
    const size_t bytes = n * (size_t)c->N;
    hipError_t err = hipSuccess;
    auto alloc = [&](auto** p, size_t sz, bool zero = false) {
        if (err == hipSuccess) err = env_alloc(e, p, sz, zero);
    };
    // every per-board field starts zeroed: a never-reset env reads back zeros, not stale device memory.
    // The fills go to the context stream and are finished before the env is handed out. As hipMemset
    // calls they ran on the null stream, which may return before the fill is done and which the
    // non-blocking context and shard streams do not wait for: a fill could land after m3_env_reset's
    // seed upload on the context stream, and the first boards of the env then reset from seed 0.
    constexpr bool ZERO = true;
    alloc(&e->boards[0], bytes, ZERO);
    alloc(&e->boards[1], bytes, ZERO);
    alloc(&e->seeds, n * 4, ZERO);
    alloc(&e->flags, n * 4, ZERO);
    alloc(&e->draws, n * 4, ZERO);
    alloc(&e->legal, n * 4ull * c->AW, ZERO);
    alloc(&e->score, n * 4, ZERO);
    alloc(&e->moves, n * 4, ZERO);
    alloc(&e->next_action, n * 4, ZERO);
    alloc(&e->reward, n * 4, ZERO);
    alloc(&e->done, n, ZERO);
    alloc(&e->trunc, n, ZERO);
    alloc(&e->slot, n, ZERO);
    // (the counters too: m3_env_stats of an env that was loaded with m3_env_set and has not stepped
    // yet -- rederive zeroes them at its first step -- read back whatever the allocation held)
    alloc(&e->counters, 64 * 4 * MAX_SHARDS, ZERO);
    alloc(&e->ovf_list, n * 4);
    alloc(&e->packed, 2 * n * 4);
    alloc(&e->ne_words, (size_t)NSLOT * n * 4ull * ((c->N + 3) / 4));
    alloc(&e->ne_first, (size_t)NSLOT * n * 4);
    alloc(&e->ne_legal, (size_t)NSLOT * n * 4ull * c->AW);
    alloc(&e->ne_flags, (size_t)NSLOT * n * 4);
    alloc(&e->defer, n * 4);
    for (int p = 0; p < PF_LAG; ++p) {
        alloc(&e->pf_list[p], n * 4);
        alloc(&e->pf_seed[p], n * 4);
        alloc(&e->pf_slot[p], n * 4);
    }
    with_shape(c->shape, [&](auto cf) {
        using K = KS<decltype(cf)>;
        using St = LdsStore<decltype(cf), K::GCAP, K::B>;
        alloc(&e->spill, (size_t)MAX_SHARDS * K::SPILL_RECORDS * St::SPILL_WORDS * 4);
        alloc(&e->m397, (size_t)NSLOT * n * 4ull);
        constexpr size_t RW = CONT_REC<decltype(cf)>;
        if constexpr (K::CASCADE_LIMIT >= 0) alloc(&e->cont, RW * n * 4ull);
        if constexpr (RESET_TWO_STAGE<decltype(cf)>) alloc(&e->tab, (size_t)TwoStage<decltype(cf)>::TW * n * 4ull);
        return 0;
    });
    for (hipEvent_t& ev : e->gev)
        if (err == hipSuccess) err = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) {
        m3_env_destroy(e);
        return set_err(M3_ERR_HIP, "env allocation (%lld boards): %s", (long long)n, hipGetErrorString(err));
    }
    // default: one shard. Every shard adds two streams (step + prefetch), and
    // streams beyond GPU_MAX_HW_QUEUES (HIP default 4) share hardware queues,
    // so a step queues behind a reset launch. Measured at 1,048,576 boards
    // (9x9x6, autoreset, gpurun_out/q1-q3): 4 queues: 1 / 2 / 4 shards = 1.75 /
    // 1.43 / 1.18 G env-steps/s; 8 queues: 1.74 / 1.98 / 1.38 (2 shards fill
    // each other's kernel tails); one prefetch stream shared by 2 shards: 1.67.
    int rc = m3_env_set_shards(e, 1);
    if (rc) {
        m3_env_destroy(e);
        return rc;
    }
    *out = e;
    return M3_OK;
}

int m3_env_set_shards(m3_env* e, int nshards) {
    CHECK_ARG(e && nshards >= 1 && nshards <= MAX_SHARDS, "nshards must be in [1, 8]");
    HIP_TRY(hipSetDevice(e->ctx->device));
    int rc = sync_env(e);
    if (rc) return rc;
    destroy_shards(e);
    // Shard slot s keeps its counter blocks across the call, and only its own k_env_fix rotates them
    // (CBLOCKS): a slot that sat out some steps comes back with the blocks of its last steps still
    // counting their overflow lists, continuation records and prefetch queues. Nothing is in flight
    // and every list of a past step is consumed, so all blocks of all slots start the next step empty;
    // the stats words behind them stay.
    for (int s = 0; s < MAX_SHARDS; ++s)
        HIP_TRY(hipMemsetAsync(e->counters + 64 * s, 0, 8 * CBLOCKS * 4, e->ctx->stream));
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    // shard boundaries on 256-board multiples
    const int64_t per = ((e->n + nshards - 1) / nshards + BLOCK - 1) / BLOCK * BLOCK;
    for (int s = 0; s < nshards; ++s) {
        m3_env::Shard sh;
        sh.off = std::min<int64_t>(e->n, s * per);
        sh.n = std::min<int64_t>(e->n, sh.off + per) - sh.off;
        HIP_TRY(hipStreamCreateWithFlags(&sh.stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&sh.pstream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&sh.ev, hipEventDisableTiming));
        for (hipEvent_t& ev : sh.pev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        for (hipEvent_t& ev : sh.aev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        e->shards.push_back(sh);
    }
    return M3_OK;
}

int m3_env_synchronize(m3_env* e) {
    CHECK_ARG(e, "null env");
    HIP_TRY(hipSetDevice(e->ctx->device));
    int rc = sync_env(e);
    if (rc) return rc;
    return ensure_fresh(e);
}

int m3_env_destroy(m3_env* e) {
    if (!e) return M3_OK;
    (void)hipSetDevice(e->ctx->device);
    (void)sync_env(e);
    destroy_shards(e);
    for (int p = 0; p < 2; ++p) {
        if (e->upload_ev[p]) (void)hipEventDestroy(e->upload_ev[p]);
        if (e->hstage[p]) (void)hipHostFree(e->hstage[p]);
    }
    if (e->ustream) (void)hipStreamDestroy(e->ustream);
    for (hipEvent_t ev : e->gev)
        if (ev) (void)hipEventDestroy(ev);
    for (void* p : e->owned) (void)hipFree(p);
    if (e->comm) ncclCommDestroy(e->comm);
    for (hipEvent_t ev : e->tev) (void)hipEventDestroy(ev);
    delete e;
    return M3_OK;
}

int m3_env_reset(m3_env* e, const uint32_t* seeds, uint32_t seed_base) {
    CHECK_ARG(e, "null env");
    m3_ctx* c = e->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc0 = sync_env(e);
    if (rc0) return rc0;
    if (seeds) {
        HIP_TRY(hipMemcpyAsync(e->seeds, seeds, e->n * 4, hipMemcpyHostToDevice, c->stream));
    } else {
        // seeds = seed_base + i, written on host once (reset is not on the hot path)
        uint32_t* h = (uint32_t*)malloc(e->n * 4);
        if (!h) return set_err(M3_ERR_INVALID, "host allocation failed");
        for (int64_t i = 0; i < e->n; ++i) h[i] = seed_base + (uint32_t)i;
        hipError_t err = hipMemcpy(e->seeds, h, e->n * 4, hipMemcpyHostToDevice);
        free(h);
        HIP_TRY(err);
    }
    InitArgs a{};
    a.shape = c->sdesc;
    a.n = e->n;
    a.seeds = e->seeds;
    a.boards = e->boards[e->cur];
    a.first_action = e->next_action;
    a.legal = e->legal;
    a.score = e->score;
    a.moves = e->moves;
    a.reward = e->reward;
    a.done = e->done;
    a.trunc = e->trunc;
    a.flags = e->flags;
    a.draws = e->draws;
    a.m397 = e->m397;
    a.cstride = e->n;
    HIP_TRY(hipMemsetAsync(e->counters, 0, 64 * 4 * MAX_SHARDS, c->stream));  // also clears the stats
    HIP_TRY(hipMemsetAsync(e->slot, 0, e->n, c->stream));
    e->steps = 0;
    int rc = with_shape(c->shape, [&](auto cf) {
        int r = launch_init<decltype(cf)>(c->stream, a, e->n);
        if (r == M3_OK && e->autoreset) r = fill_next_slots<decltype(cf)>(e);
        return r;
    });
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    e->ready = true;
    e->stale = false;
    return M3_OK;
}

int m3_env_set_autoreset(m3_env* e, int enabled, uint32_t seed_stride) {
    CHECK_ARG(e, "null env");
    HIP_TRY(hipSetDevice(e->ctx->device));
    int rc = sync_env(e);
    if (rc) return rc;
    const bool refill = enabled && e->ready && (!e->autoreset || e->stride != seed_stride);
    e->autoreset = enabled ? 1 : 0;
    e->stride = seed_stride;
    if (refill)  // the queued next episodes depend on the stride
        return with_shape(e->ctx->shape, [&](auto cf) { return fill_next_slots<decltype(cf)>(e); });
    return M3_OK;
}

int m3_env_step_device(m3_env* e, const int32_t* d_actions) {
    CHECK_ARG(e, "null env");
    if (!e->ready) return not_ready_error("m3_env_step");
    HIP_TRY(hipSetDevice(e->ctx->device));
    return with_shape(e->ctx->shape, [&](auto cf) {
        if (e->stale) {
            const int rc = rederive<decltype(cf)>(e);
            if (rc) return rc;
        }
        return launch_env_step<decltype(cf)>(e, d_actions);
    });
}

// Host actions: copied into pinned staging[p] (p = step parity) on the host,
// uploaded to actions[p] on the upload stream, which waits only for the
// shards of step t-2 (the last readers of actions[p]) -- not for step t-1 and
// not for an RCCL gather on the context stream. The host blocks only until
// the upload of step t-2 has left staging[p].
int m3_env_step(m3_env* e, const int32_t* actions) {
    CHECK_ARG(e, "null env");
    if (!actions) return m3_env_step_device(e, nullptr);
    if (!e->ready) return not_ready_error("m3_env_step");
    HIP_TRY(hipSetDevice(e->ctx->device));
    // a loaded env rederives (and restarts the step counter) before the upload buffer's parity is
    // chosen: the kernel of this step reads actions[steps & 1] of the counter it runs under
    int rc0 = ensure_fresh(e);
    if (rc0) return rc0;
    const size_t bytes = (size_t)e->n * 4;
    if (!e->ustream) {
        HIP_TRY(hipStreamCreateWithFlags(&e->ustream, hipStreamNonBlocking));
        for (int p = 0; p < 2; ++p) {
            HIP_TRY(hipEventCreateWithFlags(&e->upload_ev[p], hipEventDisableTiming));
            HIP_TRY(env_alloc(e, &e->actions[p], bytes, false));
            HIP_TRY(hipHostMalloc(&e->hstage[p], bytes, hipHostMallocDefault));
        }
    }
    const int pb = (int)(e->steps & 1);
    if (e->upload_pend[pb]) {  // staging[pb] still feeding the upload of step t-2
        HIP_TRY(hipEventSynchronize(e->upload_ev[pb]));
        e->upload_pend[pb] = false;
    }
    memcpy(e->hstage[pb], actions, bytes);
    for (auto& sh : e->shards)
        if (sh.n && sh.apending[pb]) HIP_TRY(hipStreamWaitEvent(e->ustream, sh.aev[pb], 0));
    HIP_TRY(hipMemcpyAsync(e->actions[pb], e->hstage[pb], bytes, hipMemcpyHostToDevice, e->ustream));
    HIP_TRY(hipEventRecord(e->upload_ev[pb], e->ustream));
    e->upload_pend[pb] = true;
    e->upload_this = true;
    const int rc = m3_env_step_device(e, e->actions[pb]);
    e->upload_this = false;
    return rc;
}

// The lookahead of the env's current boards, per shard on the shard's step stream: behind the
// previous step's k_env_step / k_env_cont_grid / k_env_fix, ahead of whatever is enqueued next.
int m3_env_lookahead(m3_env* e, int32_t* d_best_action, int32_t* d_best_reward, int32_t* d_values) {
    CHECK_ARG(e, "null env");
    if (!e->ready) return not_ready_error("m3_env_lookahead");
    m3_ctx* c = e->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_fresh(e);
    if (rc) return rc;
    if (!e->look_list) {
        HIP_TRY(env_alloc(e, &e->look_list, e->n * 4, false));
        HIP_TRY(env_alloc(e, &e->look_cnt, MAX_SHARDS * 4, false));
    }
    for (int s = 0; s < (int)e->shards.size(); ++s) {
        m3_env::Shard& sh = e->shards[s];
        if (sh.n == 0) continue;
        const int64_t o = sh.off;
        LookArgs a{};
        a.shape = c->sdesc;
        a.n = sh.n;
        a.boards = e->boards[e->cur] + o * c->N;
        a.seeds = e->seeds + o;
        a.moves = e->moves + o;
        a.num_moves = e->num_moves;
        a.best_action = d_best_action ? d_best_action + o : nullptr;
        a.best_reward = d_best_reward ? d_best_reward + o : nullptr;
        a.values = d_values ? d_values + o * c->A : nullptr;
        a.ovf_count = e->look_cnt + s;
        a.ovf_list = e->look_list + o;
        HIP_TRY(hipMemsetAsync(a.ovf_count, 0, 4, sh.stream));
        rc = with_shape(c->shape, [&](auto cf) { return launch_lookahead<decltype(cf)>(sh.stream, a); });
        if (rc) return rc;
        HIP_TRY(hipEventRecord(sh.ev, sh.stream));  // (the shard's last work: m3_env_get joins on it)
    }
    return M3_OK;
}

int m3_env_step_greedy(m3_env* e) {
    CHECK_ARG(e, "null env");
    if (!e->ready) return not_ready_error("m3_env_step_greedy");
    HIP_TRY(hipSetDevice(e->ctx->device));
    if (!e->look_act) HIP_TRY(env_alloc(e, &e->look_act, e->n * 4, false));
    // (each shard's step kernel follows its lookahead on the same stream, and the lookahead of the
    // next step follows the step: look_act needs no double buffer)
    int rc = m3_env_lookahead(e, e->look_act, nullptr, nullptr);
    if (rc) return rc;
    return m3_env_step_device(e, e->look_act);
}

static int env_field(m3_env* e, int what, void** ptr, size_t* bytes) {
    const int64_t n = e->n;
    switch (what) {
        case M3_ENV_BOARDS: *ptr = e->boards[e->cur]; *bytes = n * (size_t)e->ctx->N; return M3_OK;
        case M3_ENV_REWARD: *ptr = e->reward; *bytes = n * 4; return M3_OK;
        case M3_ENV_DONE: *ptr = e->done; *bytes = n; return M3_OK;
        case M3_ENV_TRUNCATED: *ptr = e->trunc; *bytes = n; return M3_OK;
        case M3_ENV_SCORE: *ptr = e->score; *bytes = n * 4; return M3_OK;
        case M3_ENV_MOVES: *ptr = e->moves; *bytes = n * 4; return M3_OK;
        case M3_ENV_FLAGS: *ptr = e->flags; *bytes = n * 4; return M3_OK;
        case M3_ENV_NEXT_ACTION: *ptr = e->next_action; *bytes = n * 4; return M3_OK;
        case M3_ENV_LEGAL: *ptr = e->legal; *bytes = n * 4ull * e->ctx->AW; return M3_OK;
        case M3_ENV_SEEDS: *ptr = e->seeds; *bytes = n * 4; return M3_OK;
        case M3_ENV_DRAWS: *ptr = e->draws; *bytes = n * 4; return M3_OK;
        case M3_ENV_GATHERED:
            if (!e->gathered) return set_err(M3_ERR_STATE, "M3_ENV_GATHERED before m3_env_comm_init");
            *ptr = e->gathered;
            *bytes = (size_t)e->nranks * n * 4;
            return M3_OK;
        default: return set_err(M3_ERR_INVALID, "unknown env field %d", what);
    }
}

int m3_env_get(m3_env* e, int what, void* host_out) {
    CHECK_ARG(e && host_out, "bad arguments");
    void* p;
    size_t bytes;
    int rc = env_field(e, what, &p, &bytes);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->ctx->device));
    rc = ensure_fresh(e);
    if (rc) return rc;
    rc = join_shards(e, e->ctx->stream);
    if (rc) return rc;
    if (what == M3_ENV_LEGAL && !e->legal_eager) {  // derived on request from the current boards
        rc = with_shape(e->ctx->shape, [&](auto cf) {
            return launch_legal<decltype(cf)>(e->ctx, e->n, e->boards[e->cur], e->legal);
        });
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(host_out, p, bytes, hipMemcpyDeviceToHost, e->ctx->stream));
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    return M3_OK;
}

int m3_env_set(m3_env* e, int what, const void* host_in) {
    CHECK_ARG(e && host_in, "bad arguments");
    switch (what) {
        case M3_ENV_BOARDS: case M3_ENV_SEEDS: case M3_ENV_SCORE: case M3_ENV_MOVES: case M3_ENV_NEXT_ACTION:
        case M3_ENV_REWARD: case M3_ENV_DONE: case M3_ENV_TRUNCATED: case M3_ENV_FLAGS: case M3_ENV_DRAWS:
            break;
        default:
            return set_err(M3_ERR_INVALID, "env field %d is derived, not settable", what);
    }
    void* p;
    size_t bytes;
    int rc = env_field(e, what, &p, &bytes);
    if (rc) return rc;
    if (what == M3_ENV_BOARDS) {
        const int8_t* b = static_cast<const int8_t*>(host_in);
        for (size_t i = 0; i < bytes; ++i)
            if (b[i] < 0) return set_err(M3_ERR_INVALID, "cell value outside [0, 127] at byte %zu", i);
    }
    HIP_TRY(hipSetDevice(e->ctx->device));
    rc = sync_env(e);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(p, host_in, bytes, hipMemcpyHostToDevice));
    e->stale = true;
    // stepping needs the whole state: after a reset any field may be overwritten; a fresh env is
    // ready once boards, seeds, score, moves and the pre-drawn action have all been loaded
    constexpr uint32_t NEED = (1u << M3_ENV_BOARDS) | (1u << M3_ENV_SEEDS) | (1u << M3_ENV_SCORE) |
                              (1u << M3_ENV_MOVES) | (1u << M3_ENV_NEXT_ACTION);
    e->loaded |= 1u << what;
    if ((e->loaded & NEED) == NEED) e->ready = true;
    return M3_OK;
}

int m3_env_comm_size(m3_env* e, int* out) {
    CHECK_ARG(e && out, "bad arguments");
    if (!e->comm) {
        *out = 1;
        return M3_OK;
    }
    int n = 0;
    RCCL_TRY(ncclCommCount(e->comm, &n));
    *out = n;
    return M3_OK;
}

int m3_env_device_ptr(m3_env* e, int what, void** out) {
    CHECK_ARG(e && out, "bad arguments");
    size_t bytes;
    int rc = env_field(e, what, out, &bytes);
    if (rc || what != M3_ENV_LEGAL || e->legal_eager) return rc;
    // a device consumer of the legal sets: from now on every step writes them; fill the buffer now
    HIP_TRY(hipSetDevice(e->ctx->device));
    rc = ensure_fresh(e);
    if (rc) return rc;
    rc = join_shards(e, e->ctx->stream);
    if (rc) return rc;
    rc = with_shape(e->ctx->shape, [&](auto cf) {
        return launch_legal<decltype(cf)>(e->ctx, e->n, e->boards[e->cur], e->legal);
    });
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    e->legal_eager = true;
    return M3_OK;
}

int m3_comm_unique_id(uint8_t out_id[128]) {
    CHECK_ARG(out_id, "null out");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    RCCL_TRY(ncclGetUniqueId(&id));
    memcpy(out_id, &id, 128);
    return M3_OK;
}

int m3_env_comm_init(m3_env* e, const uint8_t id[128], int nranks, int rank) {
    CHECK_ARG(e && id && nranks >= 1 && rank >= 0 && rank < nranks, "bad arguments");
    if (e->comm) return set_err(M3_ERR_STATE, "m3_env_comm_init: the env already has a communicator");
    HIP_TRY(hipSetDevice(e->ctx->device));
    HIP_TRY(env_alloc(e, &e->gathered, (size_t)nranks * e->n * 4, false));
    ncclUniqueId uid;
    memcpy(&uid, id, 128);
    ncclComm_t comm = nullptr;
    const ncclResult_t r = ncclCommInitRank(&comm, nranks, uid, rank);
    if (r != ncclSuccess) {  // no communicator, no buffer: take back the allocation just recorded
        e->owned.pop_back();
        (void)hipFree(e->gathered);
        e->gathered = nullptr;
        return set_err(M3_ERR_RCCL, "ncclCommInitRank: %s", ncclGetErrorString(r));
    }
    e->comm = comm;
    e->nranks = nranks;
    e->rank = rank;
    return M3_OK;
}

// ncclAllGather of the last step's packed words on the context stream into
// d_out (nullptr: the env's own buffer, M3_ENV_GATHERED).
static int env_gather(m3_env* e, int32_t* d_out) {
    if (!e->comm) return set_err(M3_ERR_STATE, "m3_env_gather before m3_env_comm_init");
    if (e->steps == 0) return set_err(M3_ERR_STATE, "m3_env_gather before the first m3_env_step");
    HIP_TRY(hipSetDevice(e->ctx->device));
    int rc = join_shards(e, e->ctx->stream);  // every shard's packed words written
    if (rc) return rc;
    const int pb = (int)((e->steps - 1) & 1);  // buffer the last step wrote
    RCCL_TRY(ncclAllGather(e->packed + (size_t)pb * e->n, d_out ? d_out : e->gathered, (size_t)e->n, ncclInt32,
                           e->comm, e->ctx->stream));
    HIP_TRY(hipEventRecord(e->gev[pb], e->ctx->stream));  // the step after next must not overwrite it early
    e->gpend[pb] = true;
    return M3_OK;
}

int m3_env_gather(m3_env* e, int32_t* host_out) {
    CHECK_ARG(e, "null env");
    int rc = env_gather(e, nullptr);
    if (rc) return rc;
    if (host_out) {
        HIP_TRY(hipMemcpyAsync(host_out, e->gathered, (size_t)e->nranks * e->n * 4, hipMemcpyDeviceToHost,
                               e->ctx->stream));
        HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    }
    return M3_OK;
}

int m3_env_gather_device(m3_env* e, int32_t* d_out) {
    CHECK_ARG(e, "null env");
    return env_gather(e, d_out);
}

}  // extern "C"

// Test hook kernel: one wave sleeping ~`rounds` x 8k cycles.
__global__ void k_stall(uint32_t rounds) {
    for (uint32_t i = 0; i < rounds; ++i) __builtin_amdgcn_s_sleep(127);
}

extern "C" {

int m3_env_debug_stall(m3_env* e, uint32_t usec) {
    CHECK_ARG(e && usec <= 10u * 1000u * 1000u, "bad arguments");
    HIP_TRY(hipSetDevice(e->ctx->device));
    // s_sleep 127 = 127 x 64 clocks, ~3.4 us at 2.4 GHz
    hipLaunchKernelGGL(k_stall, dim3(1), dim3(64), 0, e->ctx->stream, (usec + 2u) / 3u);
    HIP_TRY(hipGetLastError());
    return M3_OK;
}

int m3_env_stats(m3_env* e, uint64_t out[4]) {
    CHECK_ARG(e && out, "bad arguments");
    HIP_TRY(hipSetDevice(e->ctx->device));
    int rc = sync_env(e);
    if (rc) return rc;
    std::vector<uint32_t> h(64 * MAX_SHARDS);
    HIP_TRY(hipMemcpy(h.data(), e->counters, h.size() * 4, hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = out[3] = 0;
    for (size_t s = 0; s < (size_t)MAX_SHARDS; ++s) {  // every slot: one not in use now may have counted earlier
        out[0] += h[64 * s + 40];  // steps recomputed (cache exhausted or > table groups)
        out[1] += h[64 * s + 42];  // resets recomputed by the wave-cooperative pass (see include/m3.h)
        out[2] += h[64 * s + 41];  // autoresets (episodes prefetched)
    }
    out[3] = e->shards.size();
    return M3_OK;
}

#ifdef M3_PHASE_PROF
// profiling build only (not part of include/m3.h): out[2][PH_N + 2], summed over the
// configurations' translation units (each has its own g_prof)
#ifdef M3_SPLIT_TU
#ifdef M3_HEADLINE_ONLY
extern "C" int m3_prof_read_0(uint64_t*, int), m3_prof_read_1(uint64_t*, int);
int m3_prof_read(uint64_t* out, int reset) {
    int (*const rd[2])(uint64_t*, int) = {m3_prof_read_0, m3_prof_read_1};
#else
extern "C" int m3_prof_read_0(uint64_t*, int), m3_prof_read_1(uint64_t*, int), m3_prof_read_2(uint64_t*, int),
    m3_prof_read_3(uint64_t*, int), m3_prof_read_4(uint64_t*, int), m3_prof_read_5(uint64_t*, int),
    m3_prof_read_6(uint64_t*, int), m3_prof_read_7(uint64_t*, int), m3_prof_read_8(uint64_t*, int),
    m3_prof_read_9(uint64_t*, int);
int m3_prof_read(uint64_t* out, int reset) {
    static_assert(N_CONFIGS == 10, "one reader per configuration");
    int (*const rd[10])(uint64_t*, int) = {m3_prof_read_0, m3_prof_read_1, m3_prof_read_2, m3_prof_read_3,
                                          m3_prof_read_4, m3_prof_read_5, m3_prof_read_6, m3_prof_read_7,
                                          m3_prof_read_8, m3_prof_read_9};
#endif
    uint64_t part[2 * PROF_SLOTS];
    for (int i = 0; i < 2 * PROF_SLOTS; ++i) out[i] = 0;
    for (auto f : rd) {
        const int rc = f(part, reset);
        if (rc < 0) return rc;
        for (int i = 0; i < 2 * PROF_SLOTS; ++i) out[i] += part[i];
    }
    return PH_N;
}
#else
int m3_prof_read(uint64_t* out, int reset) { return m3_prof_read_tu(out, reset); }
#endif
#endif

// Device time of whatever is enqueued on the context stream between the two marks.
int m3_ctx_timer(m3_ctx* c, int what, float* out_ms) {
    CHECK_ARG(c && what >= 0 && what <= 1 && (what == 0 || out_ms), "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    for (hipEvent_t& ev : c->tev)
        if (!ev) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipEventRecord(c->tev[what], c->stream));
    if (what == 1) {
        HIP_TRY(hipEventSynchronize(c->tev[1]));
        HIP_TRY(hipEventElapsedTime(out_ms, c->tev[0], c->tev[1]));
    }
    return M3_OK;
}

int m3_env_timing(m3_env* e, int capacity) {
    CHECK_ARG(e && capacity >= 0, "bad arguments");
    HIP_TRY(hipSetDevice(e->ctx->device));
    int rc = sync_env(e);
    if (rc) return rc;
    while ((int)e->tev.size() < 3 * capacity) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        e->tev.push_back(ev);
    }
    e->tcap = capacity;
    e->tn = 0;
    return M3_OK;
}

int m3_env_kernel_ms(m3_env* e, float* out_ms, int max_n, int* out_n) {
    CHECK_ARG(e && out_n && (max_n == 0 || out_ms), "bad arguments");
    HIP_TRY(hipSetDevice(e->ctx->device));
    const int n = e->tn < max_n ? e->tn : max_n;
    int rc = sync_env(e);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) HIP_TRY(hipEventElapsedTime(&out_ms[i], e->tev[3 * i], e->tev[3 * i + 2]));
    *out_n = n;
    return M3_OK;
}

int m3_env_step_kernel_ms(m3_env* e, float* out_ms, int max_n, int* out_n) {
    CHECK_ARG(e && out_n && (max_n == 0 || out_ms), "bad arguments");
    HIP_TRY(hipSetDevice(e->ctx->device));
    const int n = e->tn < max_n ? e->tn : max_n;
    int rc = sync_env(e);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) HIP_TRY(hipEventElapsedTime(&out_ms[i], e->tev[3 * i], e->tev[3 * i + 1]));
    *out_n = n;
    return M3_OK;
}

}  // extern "C"

// ---- device-resident MCTS trees (m3_search.hpp: the tree kernels) -------------
struct m3_search {
    m3_ctx* ctx = nullptr;
    int64_t n = 0;
    int32_t cap = 0;
    bool ready = false;
    int64_t used = 0;  // nodes below the root ever attached, per game at most (m3s::search_run_fits)
    m3s::SearchRound R{};
    uint32_t* seeds = nullptr;  // [n] cfg.seed of each game
    // the rest of the apply and rollout launches' outputs
    int8_t* out_boards = nullptr;
    int32_t* out_reward = nullptr;
    uint32_t *out_draws = nullptr, *out_flags = nullptr, *out_legal = nullptr, *apply_list = nullptr;
    int32_t *ro_gain = nullptr, *ro_steps = nullptr;
    uint32_t *ro_draws = nullptr, *ro_flags = nullptr;
    char* ro_tail = nullptr;       // rollout_tail_bytes: the exact pass's list and the spill pool
    uint32_t* counters = nullptr;  // [0] the apply launch's overflow count, [4..7] the rollout launch's counters
    int32_t* keep_best = nullptr;  // [n] best_action of the last m3_search_result
    uint64_t* stats = nullptr;
    hipEvent_t up_ev = nullptr;    // the rollout seeds of a run have left the pinned staging
    std::vector<void*> owned;
};

namespace {

template <class T>
hipError_t search_alloc(m3_search* s, T** field, size_t bytes) {
    hipError_t err = hipMalloc((void**)field, bytes ? bytes : 4);
    if (err == hipSuccess) s->owned.push_back(*field);
    return err;
}

// One simulation round on the context stream (rollout = false: the constructor's expansion only).
int enqueue_search_round(m3_search* s, const uint32_t* d_rseeds, bool rollout) {
    m3_ctx* c = s->ctx;
    HIP_TRY(m3s::launch_search_select(c->stream, s->R));
    ApplyArgs a{};
    a.shape = c->sdesc;
    a.n = s->n;
    a.boards = s->R.row_boards;
    a.seeds = s->seeds;
    a.n_actions = s->R.row_na;
    a.actions = s->R.T.action;
    a.out_boards = s->out_boards;
    a.reward = s->out_reward;
    a.draws = s->out_draws;
    a.flags = s->out_flags;
    a.legal = s->out_legal;
    a.ovf_count = s->counters;
    a.ovf_list = s->apply_list;
    int rc = with_shape(c->shape, [&](auto cf) { return launch_apply<decltype(cf)>(c, a); });
    if (rc) return rc;
    HIP_TRY(m3s::launch_search_attach(c->stream, s->R));
    if (!rollout) return M3_OK;
    RolloutArgs r{};
    r.n = s->n;
    r.boards = s->R.ro_boards;
    r.seeds = s->seeds;
    r.n_actions = s->R.ro_na;
    r.rseeds = d_rseeds;
    r.gain = s->ro_gain;
    r.steps = s->ro_steps;
    r.draws = s->ro_draws;
    r.flags = s->ro_flags;
    rc = enqueue_rollouts(c, r, s->ro_tail, s->counters + 4);
    if (rc) return rc;
    HIP_TRY(m3s::launch_search_backup(c->stream, s->R));
    return M3_OK;
}

int search_not_ready(const char* entry) { return set_err(M3_ERR_STATE, "%s before m3_search_set_roots", entry); }

}  // namespace

extern "C" {

int m3_search_log_table(int32_t n, double* out) {
    CHECK_ARG(n >= 0 && (n == 0 || out), "bad arguments");
    std::vector<double> tab((size_t)n + 1);
    m3s::search_log_table(n, tab.data());
    for (int32_t v = 1; v <= n; ++v) out[v - 1] = tab[v];
    return M3_OK;
}

int m3_search_create(m3_ctx* c, int64_t n, int32_t node_capacity, m3_search** out) {
    CHECK_ARG(c && out && n > 0 && node_capacity >= 2, "bad arguments");
    CHECK_ARG(n < (int64_t)1 << 31, "n too large");
    *out = nullptr;
    int rc = check_ids_on_board(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    m3_search* s = new m3_search;
    s->ctx = c;
    s->n = n;
    s->cap = node_capacity;
    m3s::STree& T = s->R.T;
    T.n = n;
    T.cap = node_capacity;
    T.N = c->N;
    T.AW = c->AW;
    T.A = c->A;
    const size_t nodes = (size_t)n * (size_t)node_capacity, bytes = (size_t)n * c->N, aw = (size_t)n * 4 * c->AW;
    hipError_t err = hipSuccess;
    auto alloc = [&](auto** p, size_t sz) {
        if (err == hipSuccess) err = search_alloc(s, p, sz);
    };
    alloc(&T.hot, nodes * sizeof(m3s::SNodeHot));
    alloc(&T.link, nodes * sizeof(m3s::SNodeLink));
    alloc(&T.untried, nodes * 4 * c->AW);
    alloc(&T.boards, nodes * c->N);
    alloc(&T.root, n * 4);
    alloc(&T.used, n * 4);
    alloc(&T.leaf, n * 4);
    alloc(&T.expanded, n * 4);
    alloc(&T.action, n * 4);
    alloc(&T.gflags, n * 4);
    double* log_tab = nullptr;
    alloc(&log_tab, ((size_t)node_capacity + 1) * 8);
    T.log_tab = log_tab;
    alloc(&s->R.row_boards, bytes);
    alloc(&s->R.row_na, n * 4);
    alloc(&s->R.ro_boards, bytes);
    alloc(&s->R.ro_na, n * 4);
    alloc(&s->seeds, n * 4);
    alloc(&s->out_boards, bytes);
    alloc(&s->out_reward, n * 4);
    alloc(&s->out_draws, n * 4);
    alloc(&s->out_flags, n * 4);
    alloc(&s->out_legal, aw);
    alloc(&s->apply_list, n * 4);
    alloc(&s->ro_gain, n * 4);
    alloc(&s->ro_steps, n * 4);
    alloc(&s->ro_draws, n * 4);
    alloc(&s->ro_flags, n * 4);
    alloc(&s->ro_tail, rollout_tail_bytes(c->shape, n));
    alloc(&s->counters, 32);
    alloc(&s->keep_best, n * 4);
    alloc(&s->stats, 32);
    s->R.out_boards = s->out_boards;
    s->R.out_reward = s->out_reward;
    s->R.out_flags = s->out_flags;
    s->R.out_legal = s->out_legal;
    s->R.ro_gain = s->ro_gain;
    s->R.ro_flags = s->ro_flags;
    s->R.apply_ovf = s->counters;
    s->R.ro_counters = s->counters + 4;
    s->R.stats = s->stats;
    std::vector<double> tab((size_t)node_capacity + 1);
    m3s::search_log_table(node_capacity, tab.data());  // log on the host only (m3_search_core.hpp)
    if (err == hipSuccess) err = hipEventCreateWithFlags(&s->up_ev, hipEventDisableTiming);
    if (err == hipSuccess) err = hipMemcpyAsync(log_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream);
    if (err == hipSuccess) err = hipMemsetAsync(s->counters, 0, 32, c->stream);
    if (err == hipSuccess) err = hipMemsetAsync(s->stats, 0, 32, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) {
        m3_search_destroy(s);
        return set_err(M3_ERR_HIP, "search allocation (%lld games x %d nodes): %s", (long long)n, node_capacity,
                       hipGetErrorString(err));
    }
    *out = s;
    return M3_OK;
}

int m3_search_destroy(m3_search* s) {
    if (!s) return M3_OK;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    for (void* p : s->owned) (void)hipFree(p);
    if (s->up_ev) (void)hipEventDestroy(s->up_ev);
    delete s;
    return M3_OK;
}

int m3_search_set_roots(m3_search* s, const int8_t* boards, const uint32_t* seeds, const int32_t* n_actions,
                        const int32_t* rewards) {
    CHECK_ARG(s && boards && seeds && n_actions && rewards, "bad arguments");
    m3_ctx* c = s->ctx;
    const int64_t n = s->n;
    for (size_t i = 0, e = (size_t)n * c->N; i < e; ++i)
        if (boards[i] < 0) return bad_cells_error();
    HIP_TRY(hipSetDevice(c->device));
    s->ready = false;
    HostCall hc(c);
    const int i_b = hc.input(boards, n * (size_t)c->N), i_s = hc.input(seeds, n * 4ull),
              i_na = hc.input(n_actions, n * 4ull), i_r = hc.input(rewards, n * 4ull);
    int rc = hc.begin(false, 16, 0);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s->seeds, hc.dev<const uint32_t>(i_s), n * 4ull, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(s->stats, 0, 32, c->stream));
    rc = with_shape(c->shape, [&](auto cf) {
        return launch_legal<decltype(cf)>(c, n, hc.dev<const int8_t>(i_b), s->out_legal);
    });
    if (rc) return rc;
    HIP_TRY(m3s::launch_search_init(c->stream, s->R.T, hc.dev<const int8_t>(i_b), hc.dev<const int32_t>(i_na),
                                    hc.dev<const int32_t>(i_r), s->out_legal));
    rc = enqueue_search_round(s, nullptr, false);  // MCTS.__init__'s one expansion (abc/mcts.py:82)
    if (rc) return rc;
    rc = hc.finish();
    if (rc) return rc;
    s->used = 1;
    s->ready = true;
    return M3_OK;
}

int m3_search_run(m3_search* s, int32_t simulations, const uint32_t* rollout_seeds) {
    CHECK_ARG(s && simulations >= 0 && (simulations == 0 || rollout_seeds), "bad arguments");
    if (!s->ready) return search_not_ready("m3_search_run");
    if (!m3s::search_run_fits(s->used, simulations, s->cap))  // before anything is enqueued
        return set_err(M3_ERR_CAP, "%d simulations on trees of up to %lld nodes do not fit node_capacity %d",
                       simulations, (long long)s->used + 1, s->cap);
    if (simulations == 0) return M3_OK;
    m3_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    HostCall hc(c);
    const int i_rs = hc.input(rollout_seeds, (size_t)simulations * s->n * 4ull);
    int rc = hc.begin(false, 0, 0);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s->up_ev, c->stream));
    s->used += simulations;
    const uint32_t* d_rs = hc.dev<const uint32_t>(i_rs);
    for (int32_t k = 0; k < simulations && rc == M3_OK; ++k) rc = enqueue_search_round(s, d_rs + (size_t)k * s->n, true);
    // the seeds have left the pinned staging (the next host-buffer call may fill it); the kernels run on
    HIP_TRY(hipEventSynchronize(s->up_ev));
    return rc;
}

int m3_search_result(m3_search* s, int32_t* best_action, int32_t* value, int32_t* root_visits, int32_t* n_children,
                     int32_t* child_action, int32_t* child_visits, int64_t* child_reward, uint32_t* flags) {
    CHECK_ARG(s, "null search");
    if (!s->ready) return search_not_ready("m3_search_result");
    m3_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)s->n, na = n * c->A;
    HostCall hc(c);
    const int o_a = hc.output(best_action, n * 4), o_v = hc.output(value, n * 4), o_rv = hc.output(root_visits, n * 4),
              o_nc = hc.output(n_children, n * 4), o_ca = hc.output(child_action, na * 4),
              o_cv = hc.output(child_visits, na * 4), o_cr = hc.output(child_reward, na * 8),
              o_f = hc.output(flags, n * 4);
    int rc = hc.begin(false, 16, 0);
    if (rc) return rc;
    m3s::SResult r{hc.dev<int32_t>(o_a),  hc.dev<int32_t>(o_v),  hc.dev<int32_t>(o_rv), hc.dev<int32_t>(o_nc),
                   hc.dev<int32_t>(o_ca), hc.dev<int32_t>(o_cv), hc.dev<int64_t>(o_cr), hc.dev<uint32_t>(o_f)};
    HIP_TRY(m3s::launch_search_finish(c->stream, s->R.T, r, s->keep_best, s->stats));
    return hc.finish();
}

int m3_search_advance(m3_search* s, const int32_t* actions, int8_t* out_boards, int32_t* out_rewards,
                      int32_t* out_n_actions, uint32_t* out_legal_bits) {
    CHECK_ARG(s, "null search");
    if (!s->ready) return search_not_ready("m3_search_advance");
    m3_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)s->n;
    std::vector<uint32_t> fl(n);
    HostCall hc(c);
    const int i_a = actions ? hc.input(actions, n * 4) : -1;
    const int o_b = hc.output(out_boards, n * c->N), o_r = hc.output(out_rewards, n * 4),
              o_na = hc.output(out_n_actions, n * 4), o_l = hc.output(out_legal_bits, n * 4 * c->AW),
              o_f = hc.output(fl.data(), n * 4);
    int rc = hc.begin(false, 16, 0);
    if (rc) return rc;
    // (outputs the caller does not want land in the round's row buffers, rewritten by the next round)
    int8_t* d_b = out_boards ? hc.dev<int8_t>(o_b) : s->R.row_boards;
    HIP_TRY(m3s::launch_search_advance(c->stream, s->R.T, actions ? hc.dev<const int32_t>(i_a) : s->keep_best, d_b,
                                       out_rewards ? hc.dev<int32_t>(o_r) : s->out_reward,
                                       out_n_actions ? hc.dev<int32_t>(o_na) : s->R.row_na, hc.dev<uint32_t>(o_f)));
    if (out_legal_bits) {
        rc = with_shape(c->shape, [&](auto cf) { return launch_legal<decltype(cf)>(c, s->n, d_b, hc.dev<uint32_t>(o_l)); });
        if (rc) return rc;
    }
    rc = hc.finish();
    if (rc) return rc;
    int64_t bad = 0;
    for (uint32_t f : fl) bad += (f & M3_FLAG_BAD_ACTION) != 0;
    if (bad)
        return set_err(M3_ERR_INVALID, "%lld of %lld games: the action has no expanded child of the root (their roots "
                       "stay; the outputs hold the current roots)", (long long)bad, (long long)n);
    return M3_OK;
}

int m3_search_stats(m3_search* s, uint64_t out[4]) {
    CHECK_ARG(s && out, "bad arguments");
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipMemcpyAsync(out, s->stats, 32, hipMemcpyDeviceToHost, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return M3_OK;
}

int m3_search_ucb1(m3_ctx* c, int64_t n, const int64_t* reward_sum, const int32_t* visits, const int32_t* parent_visits,
                   const double* cw, double* out) {
    CHECK_ARG(c && n >= 0, "bad arguments");
    if (n == 0) return M3_OK;
    CHECK_ARG(reward_sum && visits && parent_visits && cw && out, "null buffer");
    int32_t top = 1;
    for (int64_t i = 0; i < n; ++i) {
        CHECK_ARG(visits[i] >= 0 && parent_visits[i] >= 1 && parent_visits[i] <= 1 << 24, "visits out of range");
        top = std::max(top, parent_visits[i]);
    }
    std::vector<double> tab((size_t)top + 1);
    m3s::search_log_table(top, tab.data());
    HIP_TRY(hipSetDevice(c->device));
    HostCall hc(c);
    const int i_r = hc.input(reward_sum, n * 8ull), i_v = hc.input(visits, n * 4ull),
              i_p = hc.input(parent_visits, n * 4ull), i_c = hc.input(cw, n * 8ull),
              i_t = hc.input(tab.data(), tab.size() * 8);
    const int o = hc.output(out, n * 8ull);
    int rc = hc.begin(false, 0, 0);
    if (rc) return rc;
    HIP_TRY(m3s::launch_search_ucb1(c->stream, n, hc.dev<const int64_t>(i_r), hc.dev<const int32_t>(i_v),
                                    hc.dev<const int32_t>(i_p), hc.dev<const double>(i_c), hc.dev<const double>(i_t),
                                    hc.dev<double>(o)));
    return hc.finish();
}

}  // extern "C"

// ---- the policy/value network (m3_net.hpp: the kernels; m3_net_core.hpp: folding and pre-pack) ------
struct m3_net {
    m3_ctx* ctx = nullptr;
    int L = 0;
    m3n::NetShape S{};
    float *stem_w = nullptr, *stem_b = nullptr;
    std::vector<uint16_t*> conv_w;  // 2L packed B operands
    std::vector<float*> conv_b;
    m3n::NetHeads H{};
    uint16_t* act[2] = {nullptr, nullptr};  // the workspace: two activation buffers of `chunk` boards
    int64_t chunk = 0;
    std::vector<void*> owned;
};

namespace {

// the workspace holds at most this many activation elements per buffer (64 MiB of bf16 each)
constexpr int64_t NET_WORK_ELEMS = (int64_t)1 << 25;

// stem and `layers` residual layers of n <= chunk boards: the result is in net->act[0]
int enqueue_net_trunk(m3_net* net, const int8_t* d_boards, int64_t n, int layers) {
    hipStream_t st = net->ctx->stream;
    HIP_TRY(m3n::launch_net_stem(st, net->S, n, d_boards, net->stem_w, net->stem_b, net->act[0]));
    for (int i = 0; i < layers; ++i) {
        HIP_TRY(m3n::launch_net_conv(st, net->S, n, net->act[0], net->conv_w[2 * i], net->conv_b[2 * i], nullptr,
                                     net->act[1]));
        HIP_TRY(m3n::launch_net_conv(st, net->S, n, net->act[1], net->conv_w[2 * i + 1], net->conv_b[2 * i + 1],
                                     net->act[0], net->act[0]));
    }
    return M3_OK;
}

// the whole network on n boards in device memory, chunk by chunk through the workspace
int enqueue_net_forward(m3_net* net, const int8_t* d_boards, const uint8_t* d_need, int64_t n, float* d_values,
                        float* d_logits) {
    for (int64_t b0 = 0; b0 < n; b0 += net->chunk) {
        const int64_t nb = std::min(net->chunk, n - b0);
        int rc = enqueue_net_trunk(net, d_boards + b0 * net->S.P, nb, net->L);
        if (rc) return rc;
        HIP_TRY(m3n::launch_net_heads(net->ctx->stream, net->S, nb, net->act[0], net->H, d_need ? d_need + b0 : nullptr,
                                      d_values + b0, d_logits + b0 * net->S.A));
    }
    return M3_OK;
}

}  // namespace

extern "C" {

int m3_net_destroy(m3_net* net) {
    if (!net) return M3_OK;
    (void)hipSetDevice(net->ctx->device);
    (void)hipStreamSynchronize(net->ctx->stream);
    for (void* p : net->owned) (void)hipFree(p);
    delete net;
    return M3_OK;
}

int m3_net_create(m3_ctx* c, int32_t rows, int32_t columns, int32_t types, int32_t layers, int32_t features,
                  double bn_eps, const float* blob, int64_t blob_len, m3_net** out) {
    CHECK_ARG(c && out && blob, "bad arguments");
    *out = nullptr;
    CHECK_ARG(rows == c->R && columns == c->C && types == c->T, "the network's board shape is not the context's");
    CHECK_ARG(layers >= 0 && bn_eps >= 0.0, "layers < 0 or bn_eps < 0");
    int rc = check_ids_on_board(c);
    if (rc) return rc;
    if (!m3n::net_features_ok(features))
        return set_err(M3_ERR_UNSUPPORTED, "features = %d: a multiple of 32 in %d..%d is supported", features,
                       m3n::NET_MIN_F, m3n::NET_MAX_F);
    const int P = c->N, A = c->A, CH = m3s::nn_onehot_width(c->T), F = features, L = layers;
    const int64_t want = m3n::net_blob_len(P, A, CH, L, F);
    if (blob_len != want)
        return set_err(M3_ERR_INVALID, "weight blob of %lld floats, expected %lld", (long long)blob_len, (long long)want);
    HIP_TRY(hipSetDevice(c->device));
    m3_net* net = new m3_net;
    net->ctx = c;
    net->L = L;
    net->S = m3n::NetShape{c->R, c->C, P, A, CH, F};
    net->chunk = std::max<int64_t>(1, NET_WORK_ELEMS / ((int64_t)P * F));
    hipError_t err = hipSuccess;
    auto upload = [&](const void* host, size_t bytes) -> void* {
        void* d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, bytes);
        if (err != hipSuccess) return nullptr;
        net->owned.push_back(d);
        err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
        return d;
    };
    const float* p = blob;
    auto take = [&](int64_t count) {
        const float* q = p;
        p += count;
        return q;
    };
    // a convolution with its BN, in the blob's order: kernel, bias, bn.{scale, bias, mean, var}
    struct Conv {
        const float *w, *b, *scale, *bias, *mean, *var;
    };
    auto take_conv = [&](int64_t rows_, int outs) {
        Conv k;
        k.w = take(rows_ * outs);
        k.b = take(outs);
        k.scale = take(outs);
        k.bias = take(outs);
        k.mean = take(outs);
        k.var = take(outs);
        return k;
    };
    std::vector<float> wf, bf;
    auto fold_f32 = [&](const Conv& k, int64_t rows_, int outs, const float** d_w, const float** d_b) {
        wf.resize((size_t)rows_ * outs);
        bf.resize(outs);
        m3n::net_fold_conv_f32(k.w, k.b, k.scale, k.bias, k.mean, k.var, bn_eps, rows_, outs, wf.data(), bf.data());
        *d_w = (const float*)upload(wf.data(), wf.size() * 4);
        *d_b = (const float*)upload(bf.data(), bf.size() * 4);
    };
    {
        const Conv k = take_conv((int64_t)9 * CH, F);
        const float *w = nullptr, *b = nullptr;
        fold_f32(k, (int64_t)9 * CH, F, &w, &b);
        net->stem_w = const_cast<float*>(w);
        net->stem_b = const_cast<float*>(b);
    }
    std::vector<uint16_t> wh((size_t)9 * F * F), wpk((size_t)9 * F * F);
    for (int i = 0; i < 2 * L; ++i) {
        const Conv k = take_conv((int64_t)9 * F, F);
        bf.resize(F);
        m3n::net_fold_conv_bf16(k.w, k.b, k.scale, k.bias, k.mean, k.var, bn_eps, (int64_t)9 * F, F, wh.data(), bf.data());
        m3n::net_pack(F, wh.data(), wpk.data());
        net->conv_w.push_back((uint16_t*)upload(wpk.data(), wpk.size() * 2));
        net->conv_b.push_back((float*)upload(bf.data(), bf.size() * 4));
    }
    {
        const Conv k = take_conv(F, 1);
        fold_f32(k, F, 1, &net->H.v_w, &net->H.v_b);
        const float* d1w = take((int64_t)P * F);
        const float* d1b = take(F);
        const float* d2w = take(F);
        const float* d2b = take(1);
        net->H.d1_w = (const float*)upload(d1w, (size_t)P * F * 4);
        net->H.d1_b = (const float*)upload(d1b, (size_t)F * 4);
        net->H.d2_w = (const float*)upload(d2w, (size_t)F * 4);
        net->H.d2_b = (const float*)upload(d2b, 4);
    }
    {
        const Conv k = take_conv(F, 2);
        fold_f32(k, F, 2, &net->H.p_w, &net->H.p_b);
        const float* pw = take((int64_t)2 * P * A);
        const float* pb = take(A);
        net->H.pd_w = (const float*)upload(pw, (size_t)2 * P * A * 4);
        net->H.pd_b = (const float*)upload(pb, (size_t)A * 4);
    }
    for (uint16_t*& a : net->act) {
        void* d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, (size_t)net->chunk * P * F * 2);
        if (err == hipSuccess) net->owned.push_back(d);
        a = (uint16_t*)d;
    }
    if (err != hipSuccess) {
        m3_net_destroy(net);
        return set_err(M3_ERR_HIP, "net allocation (%d layers x %d features): %s", L, F, hipGetErrorString(err));
    }
    *out = net;
    return M3_OK;
}

int m3_net_forward_device(m3_net* net, const int8_t* d_boards, const uint8_t* d_need, int64_t n, float* d_values,
                          float* d_logits) {
    CHECK_ARG(net && n >= 0, "bad arguments");
    if (n == 0) return M3_OK;
    CHECK_ARG(d_boards && d_values && d_logits, "null device array");
    HIP_TRY(hipSetDevice(net->ctx->device));
    return enqueue_net_forward(net, d_boards, d_need, n, d_values, d_logits);
}

int m3_net_forward(m3_net* net, const int8_t* boards, int64_t n, float* values, float* logits) {
    CHECK_ARG(net && n >= 0, "bad arguments");
    if (n == 0) return M3_OK;
    CHECK_ARG(boards && values && logits, "null array");
    m3_ctx* c = net->ctx;
    HIP_TRY(hipSetDevice(c->device));
    HostCall hc(c);
    const int i_b = hc.input(boards, (size_t)n * c->N);
    const int o_v = hc.output(values, (size_t)n * 4), o_l = hc.output(logits, (size_t)n * c->A * 4);
    int rc = hc.begin(false, 0, 0);
    if (rc) return rc;
    rc = enqueue_net_forward(net, hc.dev<const int8_t>(i_b), nullptr, n, hc.dev<float>(o_v), hc.dev<float>(o_l));
    if (rc) return rc;
    return hc.finish();
}

int m3_net_trunk(m3_net* net, const int8_t* boards, int64_t n, int32_t upto, float* out) {
    CHECK_ARG(net && n >= 0, "bad arguments");
    CHECK_ARG(upto >= 0 && upto <= net->L, "upto outside [0, layers]");
    if (n == 0) return M3_OK;
    CHECK_ARG(boards && out, "null array");
    m3_ctx* c = net->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t per = (int64_t)c->N * net->S.F;
    HostCall hc(c);
    const int i_b = hc.input(boards, (size_t)n * c->N);
    const int o_x = hc.output(out, (size_t)n * per * 4);
    int rc = hc.begin(false, 0, 0);
    if (rc) return rc;
    for (int64_t b0 = 0; b0 < n; b0 += net->chunk) {
        const int64_t nb = std::min(net->chunk, n - b0);
        rc = enqueue_net_trunk(net, hc.dev<const int8_t>(i_b) + b0 * c->N, nb, upto);
        if (rc) return rc;
        HIP_TRY(m3n::launch_net_widen(c->stream, nb * per, net->act[0], hc.dev<float>(o_x) + b0 * per));
    }
    return hc.finish();
}

}  // extern "C"

// ---- network-guided device MCTS trees (m3_search_nn.hpp: the tree kernels) -------------
struct m3_search_nn {
    m3_ctx* ctx = nullptr;
    int64_t n = 0;
    int32_t cap = 0;
    bool ready = false;
    int phase = 0;         // batches handed out since set_roots: 0 the roots', 1 the construction's expansion, 2 simulations
    bool pending = false;  // a batch is out and not fed yet
    int64_t used = 0;      // nodes below the root ever attached, per game at most (m3s::search_run_fits)
    m3s::NNRound R{};
    uint32_t* seeds = nullptr;  // [n] cfg.seed of each game
    int8_t* out_boards = nullptr;
    int32_t* out_reward = nullptr;
    uint32_t *out_draws = nullptr, *out_flags = nullptr, *out_legal = nullptr, *apply_list = nullptr;
    uint32_t* counters = nullptr;  // [0] the apply launch's overflow count
    int32_t* keep_best = nullptr;  // [n] best_action of the last m3_search_nn_result
    uint64_t* stats = nullptr;
    float *lin_values = nullptr, *lin_logits = nullptr;  // the built-in evaluator's answer
    uint64_t fed_host = 0, fed_device = 0, fed_linear = 0;
    std::vector<void*> owned;
};

namespace {

template <class T>
hipError_t nn_alloc(m3_search_nn* s, T** field, size_t bytes) {
    hipError_t err = hipMalloc((void**)field, bytes ? bytes : 4);
    if (err == hipSuccess) s->owned.push_back(*field);
    return err;
}

// The launches up to the next evaluation batch (the roots' batch is written by m3_search_nn_set_roots).
int enqueue_nn_batch(m3_search_nn* s) {
    if (s->phase == 0) return M3_OK;
    m3_ctx* c = s->ctx;
    HIP_TRY(m3s::launch_nn_select(c->stream, s->R));
    ApplyArgs a{};
    a.shape = c->sdesc;
    a.n = s->n;
    a.boards = s->R.row_boards;
    a.seeds = s->seeds;
    a.n_actions = s->R.row_na;
    a.actions = s->R.T.action;
    a.out_boards = s->out_boards;
    a.reward = s->out_reward;
    a.draws = s->out_draws;
    a.flags = s->out_flags;
    a.legal = s->out_legal;
    a.ovf_count = s->counters;
    a.ovf_list = s->apply_list;
    int rc = with_shape(c->shape, [&](auto cf) { return launch_apply<decltype(cf)>(c, a); });
    if (rc) return rc;
    HIP_TRY(m3s::launch_nn_attach(c->stream, s->R));
    return M3_OK;
}

// the rest of the round once the evaluator's answer is in device memory
int enqueue_nn_commit(m3_search_nn* s, const float* d_values, const float* d_logits) {
    const bool sim = s->phase >= 2;
    HIP_TRY(m3s::launch_nn_commit(s->ctx->stream, s->R, d_values, d_logits, sim ? 1 : 0));
    if (sim) s->used += 1;
    else s->phase += 1;
    s->pending = false;
    return M3_OK;
}

int nn_fits(m3_search_nn* s, int32_t simulations) {
    if (m3s::search_run_fits(s->used, simulations, s->cap)) return M3_OK;
    return set_err(M3_ERR_CAP, "%d simulations on trees of up to %lld nodes do not fit node_capacity %d", simulations,
                   (long long)s->used + 1, s->cap);
}

int nn_state(const m3_search_nn* s, const char* entry, bool want_pending) {
    if (!s->ready) return set_err(M3_ERR_STATE, "%s before m3_search_nn_set_roots", entry);
    if (s->pending != want_pending)
        return set_err(M3_ERR_STATE, want_pending ? "%s without a pending batch (m3_search_nn_batch first)"
                                                  : "%s while a batch is pending (feed it first)", entry);
    return M3_OK;
}

}  // namespace

extern "C" {

int m3_search_nn_create(m3_ctx* c, int64_t n, int32_t node_capacity, m3_search_nn** out) {
    CHECK_ARG(c && out && n > 0 && node_capacity >= 2, "bad arguments");
    CHECK_ARG(n < (int64_t)1 << 31, "n too large");
    *out = nullptr;
    int rc = check_ids_on_board(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    m3_search_nn* s = new m3_search_nn;
    s->ctx = c;
    s->n = n;
    s->cap = node_capacity;
    m3s::NTree& T = s->R.T;
    T.n = n;
    T.cap = node_capacity;
    T.N = c->N;
    T.AW = c->AW;
    T.A = c->A;
    const size_t nodes = (size_t)n * (size_t)node_capacity, bytes = (size_t)n * c->N, aw = (size_t)n * 4 * c->AW;
    hipError_t err = hipSuccess;
    auto alloc = [&](auto** p, size_t sz) {
        if (err == hipSuccess) err = nn_alloc(s, p, sz);
    };
    alloc(&T.hot, nodes * sizeof(m3s::NNodeHot));
    alloc(&T.link, nodes * sizeof(m3s::SNodeLink));
    alloc(&T.untried, nodes * 4 * c->AW);
    alloc(&T.boards, nodes * c->N);
    alloc(&T.logits, nodes * 4 * c->A);
    alloc(&T.root, n * 4);
    alloc(&T.used, n * 4);
    alloc(&T.leaf, n * 4);
    alloc(&T.expanded, n * 4);
    alloc(&T.action, n * 4);
    alloc(&T.pending, n * 4);
    alloc(&T.gflags, n * 4);
    double* log_tab = nullptr;
    alloc(&log_tab, ((size_t)node_capacity + 1) * 8);
    T.log_tab = log_tab;
    alloc(&s->R.row_boards, bytes);
    alloc(&s->R.row_na, n * 4);
    alloc(&s->R.ev_boards, bytes);
    alloc(&s->R.ev_need, n);
    alloc(&s->seeds, n * 4);
    alloc(&s->out_boards, bytes);
    alloc(&s->out_reward, n * 4);
    alloc(&s->out_draws, n * 4);
    alloc(&s->out_flags, n * 4);
    alloc(&s->out_legal, aw);
    alloc(&s->apply_list, n * 4);
    alloc(&s->counters, 32);
    alloc(&s->keep_best, n * 4);
    alloc(&s->stats, 32);
    alloc(&s->lin_values, n * 4);
    alloc(&s->lin_logits, (size_t)n * 4 * c->A);
    s->R.out_boards = s->out_boards;
    s->R.out_reward = s->out_reward;
    s->R.out_flags = s->out_flags;
    s->R.out_legal = s->out_legal;
    s->R.apply_ovf = s->counters;
    s->R.stats = s->stats;
    std::vector<double> tab((size_t)node_capacity + 1);
    m3s::search_log_table(node_capacity, tab.data());  // log on the host only (m3_search_core.hpp)
    if (err == hipSuccess) err = hipMemcpyAsync(log_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream);
    if (err == hipSuccess) err = hipMemsetAsync(s->counters, 0, 32, c->stream);
    if (err == hipSuccess) err = hipMemsetAsync(s->stats, 0, 32, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) {
        m3_search_nn_destroy(s);
        return set_err(M3_ERR_HIP, "search_nn allocation (%lld games x %d nodes): %s", (long long)n, node_capacity,
                       hipGetErrorString(err));
    }
    *out = s;
    return M3_OK;
}

int m3_search_nn_destroy(m3_search_nn* s) {
    if (!s) return M3_OK;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    for (void* p : s->owned) (void)hipFree(p);
    delete s;
    return M3_OK;
}

int m3_search_nn_set_roots(m3_search_nn* s, const int8_t* boards, const uint32_t* seeds, const int32_t* n_actions,
                           const int32_t* rewards) {
    CHECK_ARG(s && boards && seeds && n_actions && rewards, "bad arguments");
    m3_ctx* c = s->ctx;
    const int64_t n = s->n;
    for (size_t i = 0, e = (size_t)n * c->N; i < e; ++i)
        if (boards[i] < 0) return bad_cells_error();
    HIP_TRY(hipSetDevice(c->device));
    s->ready = false;
    HostCall hc(c);
    const int i_b = hc.input(boards, n * (size_t)c->N), i_s = hc.input(seeds, n * 4ull),
              i_na = hc.input(n_actions, n * 4ull), i_r = hc.input(rewards, n * 4ull);
    int rc = hc.begin(false, 16, 0);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s->seeds, hc.dev<const uint32_t>(i_s), n * 4ull, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(s->stats, 0, 32, c->stream));
    rc = with_shape(c->shape, [&](auto cf) {
        return launch_legal<decltype(cf)>(c, n, hc.dev<const int8_t>(i_b), s->out_legal);
    });
    if (rc) return rc;
    HIP_TRY(m3s::launch_nn_init(c->stream, s->R, hc.dev<const int8_t>(i_b), hc.dev<const int32_t>(i_na),
                                hc.dev<const int32_t>(i_r), s->out_legal));
    rc = hc.finish();
    if (rc) return rc;
    s->used = 1;
    s->phase = 0;
    s->pending = false;
    s->fed_host = s->fed_device = s->fed_linear = 0;
    s->ready = true;
    return M3_OK;
}

int m3_search_nn_batch(m3_search_nn* s, int32_t remaining, const int8_t** d_boards, const uint8_t** d_need) {
    CHECK_ARG(s && d_boards && d_need, "bad arguments");
    int rc = nn_state(s, "m3_search_nn_batch", false);
    if (rc) return rc;
    if (s->phase >= 2) {
        CHECK_ARG(remaining >= 1, "remaining < 1 for a simulation round");
        rc = nn_fits(s, remaining);  // before anything is enqueued
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(s->ctx->device));
    rc = enqueue_nn_batch(s);
    if (rc) return rc;
    s->pending = true;
    *d_boards = s->R.ev_boards;
    *d_need = s->R.ev_need;
    return M3_OK;
}

int m3_search_nn_feed_device(m3_search_nn* s, const float* d_values, const float* d_logits) {
    CHECK_ARG(s && d_values && d_logits, "bad arguments");
    int rc = nn_state(s, "m3_search_nn_feed_device", true);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->ctx->device));
    rc = enqueue_nn_commit(s, d_values, d_logits);
    if (rc == M3_OK) s->fed_device += 1;
    return rc;
}

int m3_search_nn_feed(m3_search_nn* s, const float* values, const float* logits) {
    CHECK_ARG(s && values && logits, "bad arguments");
    int rc = nn_state(s, "m3_search_nn_feed", true);
    if (rc) return rc;
    m3_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    HostCall hc(c);
    const int i_v = hc.input(values, (size_t)s->n * 4), i_l = hc.input(logits, (size_t)s->n * c->A * 4);
    rc = hc.begin(false, 0, 0);
    if (rc) return rc;
    rc = enqueue_nn_commit(s, hc.dev<const float>(i_v), hc.dev<const float>(i_l));
    if (rc) return rc;
    s->fed_host += 1;
    return hc.finish();  // the staging is the context's: the kernel has read it when this returns
}

int m3_search_nn_run_linear(m3_search_nn* s, int32_t simulations, const float* d_W) {
    CHECK_ARG(s && simulations >= 0 && d_W, "bad arguments");
    int rc = nn_state(s, "m3_search_nn_run_linear", false);
    if (rc) return rc;
    rc = nn_fits(s, simulations);  // before anything is enqueued
    if (rc) return rc;
    m3_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int CH = m3s::nn_onehot_width(c->T);
    int32_t left = simulations;
    while (s->phase < 2 || left > 0) {
        if (s->phase >= 2) --left;
        rc = enqueue_nn_batch(s);
        if (rc) return rc;
        HIP_TRY(m3s::launch_nn_linear(c->stream, s->R, CH, d_W, s->lin_values, s->lin_logits));
        rc = enqueue_nn_commit(s, s->lin_values, s->lin_logits);
        if (rc) return rc;
        s->fed_linear += 1;
    }
    return M3_OK;
}

int m3_search_nn_run_net(m3_search_nn* s, int32_t simulations, m3_net* net) {
    CHECK_ARG(s && simulations >= 0 && net, "bad arguments");
    int rc = nn_state(s, "m3_search_nn_run_net", false);
    if (rc) return rc;
    m3_ctx* c = s->ctx;
    if (net->ctx != c)
        return set_err(M3_ERR_INVALID, "the net was made for a %d x %d x %d context, the search for %d x %d x %d (they "
                       "must share one m3_ctx)", net->ctx->R, net->ctx->C, net->ctx->T, c->R, c->C, c->T);
    rc = nn_fits(s, simulations);  // before anything is enqueued
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int32_t left = simulations;
    while (s->phase < 2 || left > 0) {
        if (s->phase >= 2) --left;
        rc = enqueue_nn_batch(s);
        if (rc) return rc;
        rc = enqueue_net_forward(net, s->R.ev_boards, s->R.ev_need, s->n, s->lin_values, s->lin_logits);
        if (rc) return rc;
        rc = enqueue_nn_commit(s, s->lin_values, s->lin_logits);
        if (rc) return rc;
        s->fed_device += 1;
    }
    return M3_OK;
}

int m3_search_nn_result(m3_search_nn* s, int32_t* best_action, int32_t* value, int32_t* root_visits, int32_t* n_children,
                        int32_t* child_action, int32_t* child_visits, float* child_value_sum, float* child_prior,
                        uint32_t* flags) {
    CHECK_ARG(s, "null search");
    int rc = nn_state(s, "m3_search_nn_result", false);
    if (rc) return rc;
    m3_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)s->n, na = n * c->A;
    HostCall hc(c);
    const int o_a = hc.output(best_action, n * 4), o_v = hc.output(value, n * 4), o_rv = hc.output(root_visits, n * 4),
              o_nc = hc.output(n_children, n * 4), o_ca = hc.output(child_action, na * 4),
              o_cv = hc.output(child_visits, na * 4), o_cs = hc.output(child_value_sum, na * 4),
              o_cp = hc.output(child_prior, na * 4), o_f = hc.output(flags, n * 4);
    rc = hc.begin(false, 16, 0);
    if (rc) return rc;
    m3s::NResult r{hc.dev<int32_t>(o_a),  hc.dev<int32_t>(o_v),  hc.dev<int32_t>(o_rv), hc.dev<int32_t>(o_nc),
                   hc.dev<int32_t>(o_ca), hc.dev<int32_t>(o_cv), hc.dev<float>(o_cs),   hc.dev<float>(o_cp),
                   hc.dev<uint32_t>(o_f)};
    HIP_TRY(m3s::launch_nn_finish(c->stream, s->R.T, r, s->keep_best, s->stats));
    return hc.finish();
}

int m3_search_nn_advance(m3_search_nn* s, const int32_t* actions, int8_t* out_boards, int32_t* out_rewards,
                         int32_t* out_n_actions, uint32_t* out_legal_bits) {
    CHECK_ARG(s, "null search");
    int rc = nn_state(s, "m3_search_nn_advance", false);
    if (rc) return rc;
    m3_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)s->n;
    std::vector<uint32_t> fl(n);
    HostCall hc(c);
    const int i_a = actions ? hc.input(actions, n * 4) : -1;
    const int o_b = hc.output(out_boards, n * c->N), o_r = hc.output(out_rewards, n * 4),
              o_na = hc.output(out_n_actions, n * 4), o_l = hc.output(out_legal_bits, n * 4 * c->AW),
              o_f = hc.output(fl.data(), n * 4);
    rc = hc.begin(false, 16, 0);
    if (rc) return rc;
    // (outputs the caller does not want land in the round's row buffers, rewritten by the next round)
    int8_t* d_b = out_boards ? hc.dev<int8_t>(o_b) : s->R.row_boards;
    HIP_TRY(m3s::launch_nn_advance(c->stream, s->R.T, actions ? hc.dev<const int32_t>(i_a) : s->keep_best, d_b,
                                   out_rewards ? hc.dev<int32_t>(o_r) : s->out_reward,
                                   out_n_actions ? hc.dev<int32_t>(o_na) : s->R.row_na, hc.dev<uint32_t>(o_f)));
    if (out_legal_bits) {
        rc = with_shape(c->shape, [&](auto cf) { return launch_legal<decltype(cf)>(c, s->n, d_b, hc.dev<uint32_t>(o_l)); });
        if (rc) return rc;
    }
    rc = hc.finish();
    if (rc) return rc;
    int64_t bad = 0;
    for (uint32_t f : fl) bad += (f & M3_FLAG_BAD_ACTION) != 0;
    if (bad)
        return set_err(M3_ERR_INVALID, "%lld of %lld games: the action has no expanded child of the root (their roots "
                       "stay; the outputs hold the current roots)", (long long)bad, (long long)n);
    return M3_OK;
}

int m3_search_nn_stats(m3_search_nn* s, uint64_t out[6]) {
    CHECK_ARG(s && out, "bad arguments");
    HIP_TRY(hipSetDevice(s->ctx->device));
    uint64_t dev[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(dev, s->stats, 32, hipMemcpyDeviceToHost, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    out[0] = dev[0];
    out[1] = dev[1];
    out[2] = dev[2];
    out[3] = s->fed_host;
    out[4] = s->fed_device;
    out[5] = s->fed_linear;
    return M3_OK;
}

}  // extern "C"
