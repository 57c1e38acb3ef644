// Compiled op bodies: TORCH_LIBRARY_IMPL(gsplat, CUDA, ...) for the forward stage ops on the critical host path of
// rasterization() / rasterization_2dgs(), calling the C-ABI of libgsplat_amd.so (INTEGRATION.md route B). Host C++ only - no
// device code here; the kernels stay behind include/gsplat_amd.h.
//
// What an op body does is what the reference's host functions do around their kernels (shape checks, output allocation
// from the inputs' options, current stream, device guard, error translation):
//   projection_ewa_3dgs_fused / _packed      gsplat/cuda/csrc/Projection.cpp:366-440, 928-941
//   intersect_offset                         gsplat/cuda/csrc/Intersect.cpp (isect_offset_encode)
//   rasterize_to_pixels_3dgs                 gsplat/cuda/csrc/Rasterization.cpp:275-365
//   projection_2dgs_fused, rasterize_to_pixels_2dgs (ext.cpp:1163-1199)
// plus the two halves of the fused tile intersection (gsplat_amd::isect_fused_{begin,finish}) and the notes that carry the
// longest tile list and the segment workspace between calls. Every other op body, the backward ones included, is Python
// (gsplat_amd/_ops.py); each op has exactly one body. Schemas are defined by _ops.py (verbatim from ext.cpp); an IMPL block
// may be loaded before or after the definitions.
#include <chrono>
#include <cstdlib>
#include <thread>
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/gsplat_amd.h"

namespace gsplat_amd {
namespace {

using at::Tensor;
using OptTensor = std::optional<Tensor>;

// ---- plumbing ----------------------------------------------------------------------------------------------------------
struct Launch { // device guard + the tensor's device's current stream (the reference's DEVICE_GUARD + getCurrentCUDAStream)
    c10::DeviceGuard guard;
    void *stream;
    explicit Launch(const Tensor &t)
        : guard(t.device()), stream((void *)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream())
    {
        TORCH_CHECK(t.is_cuda(), "gsplat_amd kernels only run on a ROCm device (got a CPU tensor); there is no CPU fallback");
    }
};

// ---- optional timing of the C-ABI calls made from here (what gsplat_amd._cabi.profile_begin / profile_end do for the Python
// bodies): a HIP event pair on the launch stream around every call whose entry point is selected. Off by default. ---------------
struct ProfRecord {
    std::string name;
    hipEvent_t a, b;
};
std::mutex g_prof_mutex;
bool g_prof_on = false;
std::set<std::string> g_prof_only; // empty = every entry point
std::vector<ProfRecord> g_prof;

struct Timed { // RAII: start event now, stop event at scope exit (after the C-ABI call has enqueued its kernels)
    hipEvent_t a = nullptr, b = nullptr;
    void *stream;
    const char *name;
    Timed(const char *fn, void *s) : stream(s), name(fn)
    {
        if (!g_prof_on) return;
        std::lock_guard<std::mutex> lock(g_prof_mutex);
        if (!g_prof_on || (!g_prof_only.empty() && !g_prof_only.count(fn))) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, (hipStream_t)stream);
    }
    ~Timed()
    {
        if (!a) return;
        (void)hipEventRecord(b, (hipStream_t)stream);
        std::lock_guard<std::mutex> lock(g_prof_mutex);
        g_prof.push_back({name, a, b});
    }
};

void check(int rc, const char *fn)
{
    if (rc == 0) return;
    const std::string msg = gsx_last_error();
    TORCH_CHECK(rc != -1, fn, ": ", msg); // GSX_ERR_ARG: an argument check, RuntimeError like the reference's TORCH_CHECK
    TORCH_CHECK(false, fn, " failed (code ", rc, "): ", msg);
}

Tensor contig(const Tensor &t) { return t.is_contiguous() ? t : t.contiguous(); }
OptTensor contig(const OptTensor &t) { return t.has_value() && t->defined() ? OptTensor(contig(*t)) : OptTensor(); }
bool has(const OptTensor &t) { return t.has_value() && t->defined(); }

void want_f32(const Tensor &t, const char *name)
{
    TORCH_CHECK(t.scalar_type() == at::kFloat, "gsplat_amd: ", name, " must be float32 (got ", t.scalar_type(),
                     "); the gfx950 kernels compute in fp32");
}
void want_f32(const OptTensor &t, const char *name)
{
    if (has(t)) want_f32(*t, name);
}

// The reference dispatches the projection ops over float AND double (AT_DISPATCH_FLOATING_TYPES, ProjectionEWA3DGSFused.cu:260,
// 686; ProjectionEWA3DGSPacked.cu:344, 733). In its double instantiation only the MEMORY type is double: the kernels load every
// value into glm float vectors / matrices (Common.h:65-70: vec3 = glm::vec<3, float>, mat3 = glm::mat<3, 3, float>), compute in
// float and widen the results on store. Same here: double tensors are narrowed, the fp32 kernels run, float outputs are widened.
bool is_f64(const Tensor &t) { return t.defined() && t.scalar_type() == at::kDouble; }
Tensor narrow32(const Tensor &t) { return t.defined() && t.scalar_type() == at::kDouble ? t.to(at::kFloat) : t; }
OptTensor narrow32(const OptTensor &t) { return has(t) ? OptTensor(narrow32(*t)) : t; }
Tensor widen64(const Tensor &t) { return t.defined() && t.scalar_type() == at::kFloat ? t.to(at::kDouble) : t; }
OptTensor widen64(const OptTensor &t) { return has(t) ? OptTensor(widen64(*t)) : t; }

template <class T> const T *cp(const Tensor &t) { return t.defined() && t.numel() ? t.const_data_ptr<T>() : nullptr; }
template <class T> const T *cp(const OptTensor &t) { return has(t) ? cp<T>(*t) : nullptr; }
template <class T> T *mp(Tensor &t) { return t.defined() && t.numel() ? t.mutable_data_ptr<T>() : nullptr; }
const float *fp(const Tensor &t) { return cp<float>(t); }
const float *fp(const OptTensor &t) { return cp<float>(t); }
int64_t prod(c10::IntArrayRef dims)
{
    int64_t p = 1;
    for (auto d : dims) p *= d;
    return p;
}

// A pinned host word that a kernel overwrites (a count the host needs for exact-length outputs): polled instead of
// synchronising the stream, so that the kernels enqueued behind the writer keep running and the caller can go on enqueuing.
// Spins while pending(word); the wait is ~10-100 us, so it yields now and then instead of pinning a core at 100 %. After
// `timeout` the stream is synchronised (never seen; keeps the wait correct if the store is not host-visible before the
// stream drains).
template <class Pending>
int64_t poll_host_word(volatile const int64_t *slot, Pending pending, c10::hip::HIPStreamMasqueradingAsCUDA stream,
                       std::chrono::seconds timeout)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spin = 0;; ++spin) {
        const int64_t v = *slot;
        if (!pending(v) && v == *slot) return v; // two equal reads: a value caught half-written cannot pass
        if ((spin & 63u) == 63u) std::this_thread::yield();
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > timeout) break;
    }
    stream.synchronize();
    return *slot;
}

// ---- projection (dense) ------------------------------------------------------------------------------------------------
std::tuple<Tensor, Tensor, Tensor, Tensor, OptTensor>
projection_ewa_3dgs_fused(const Tensor &means_, const OptTensor &covars_, const OptTensor &quats_, const OptTensor &scales_,
                          const OptTensor &opacities_, const Tensor &viewmats_, const Tensor &Ks_, int64_t width,
                          int64_t height, double eps2d, double near_plane, double far_plane, double radius_clip,
                          bool calc_compensations, int64_t camera_model)
{
    if (is_f64(means_)) { // the double instantiation: double in memory, float arithmetic (see narrow32)
        auto [radii, m2, dep, con, comp] = projection_ewa_3dgs_fused(
            narrow32(means_), narrow32(covars_), narrow32(quats_), narrow32(scales_), narrow32(opacities_), narrow32(viewmats_),
            narrow32(Ks_), width, height, eps2d, near_plane, far_plane, radius_clip, calc_compensations, camera_model);
        return {radii, widen64(m2), widen64(dep), widen64(con), widen64(comp)};
    }
    want_f32(means_, "means"); want_f32(covars_, "covars"); want_f32(quats_, "quats"); want_f32(scales_, "scales");
    want_f32(viewmats_, "viewmats"); want_f32(Ks_, "Ks");
    TORCH_CHECK(has(covars_) || (has(quats_) && has(scales_)), "projection: either covars or (quats, scales) must be given");
    const Tensor means = contig(means_), viewmats = contig(viewmats_), Ks = contig(Ks_);
    const OptTensor covars = contig(covars_), opac = contig(opacities_);
    const OptTensor quats = has(covars) ? OptTensor() : contig(quats_), scales = has(covars) ? OptTensor() : contig(scales_);
    auto batch = means.sizes().slice(0, means.dim() - 2);
    const int64_t B = prod(batch), C = viewmats.size(-3), N = means.size(-2);
    std::vector<int64_t> shape(batch.begin(), batch.end());
    shape.push_back(C); shape.push_back(N);
    auto with = [&](int64_t last) { auto s = shape; s.push_back(last); return s; };
    Tensor radii = at::empty(with(2), means.options().dtype(at::kInt));
    Tensor means2d = at::empty(with(2), means.options()), depths = at::empty(shape, means.options());
    Tensor conics = at::empty(with(3), means.options());
    OptTensor comps;
    if (calc_compensations) comps = at::empty(shape, means.options());
    if (B * C * N == 0) return {radii, means2d, depths, conics, comps}; // nothing to launch (before the device is touched)
    Launch L(means_);
    { Timed timed_("gsx_project_ewa_fwd", L.stream); check(gsx_project_ewa_fwd(fp(means), fp(covars), fp(quats), fp(scales), fp(opac), fp(viewmats), fp(Ks), (uint32_t)B,
                              (uint32_t)C, (uint32_t)N, (uint32_t)width, (uint32_t)height, (float)eps2d, (float)near_plane,
                              (float)far_plane, (float)radius_clip, (int)camera_model, mp<int32_t>(radii), mp<float>(means2d),
                              mp<float>(depths), mp<float>(conics), comps ? mp<float>(*comps) : nullptr, L.stream),
          "gsx_project_ewa_fwd"); }
    return {radii, means2d, depths, conics, comps};
}

// ---- projection (packed rows) ----------------------------------------------------------------------------------------------
// Two passes (count -> scan -> write) and ONE host round trip for the exact number of rows (Projection.cpp:928-941). When the
// upper bound (every (image, Gaussian) pair visible) is small next to the model, the write pass is enqueued into row buffers
// of that size BEFORE the host learns nnz - it only needs the device-side offsets - and the first nnz rows are handed out:
// the GPU does not idle through the round trip, the allocations and the launch. Larger scenes allocate exact lengths
// (saving that memory is what packed rows are for).
constexpr int64_t kPackedRowBytes = 64, kPackedPreallocLimit = 1ll << 30;

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, OptTensor>
projection_ewa_3dgs_packed(const Tensor &means_, const OptTensor &covars_, const OptTensor &quats_, const OptTensor &scales_,
                           const OptTensor &opacities_, const Tensor &viewmats_, const Tensor &Ks_, int64_t width,
                           int64_t height, double eps2d, double near_plane, double far_plane, double radius_clip,
                           bool sparse_grad, bool calc_compensations, int64_t camera_model)
{
    if (is_f64(means_)) { // the double instantiation: double in memory, float arithmetic (see narrow32)
        auto [bi, ci, gi, ip, radii, m2, dep, con, comp] = projection_ewa_3dgs_packed(
            narrow32(means_), narrow32(covars_), narrow32(quats_), narrow32(scales_), narrow32(opacities_), narrow32(viewmats_),
            narrow32(Ks_), width, height, eps2d, near_plane, far_plane, radius_clip, sparse_grad, calc_compensations, camera_model);
        return {bi, ci, gi, ip, radii, widen64(m2), widen64(dep), widen64(con), widen64(comp)};
    }
    (void)sparse_grad;
    want_f32(means_, "means"); want_f32(covars_, "covars"); want_f32(quats_, "quats"); want_f32(scales_, "scales");
    want_f32(viewmats_, "viewmats"); want_f32(Ks_, "Ks");
    TORCH_CHECK(has(covars_) || (has(quats_) && has(scales_)), "projection: either covars or (quats, scales) must be given");
    const Tensor means = contig(means_), viewmats = contig(viewmats_), Ks = contig(Ks_);
    const OptTensor covars = contig(covars_), opac = contig(opacities_);
    const OptTensor quats = has(covars) ? OptTensor() : contig(quats_), scales = has(covars) ? OptTensor() : contig(scales_);
    const int64_t B = prod(means.sizes().slice(0, means.dim() - 2)), C = viewmats.size(-3), N = means.size(-2);
    const int64_t total = B * C * N;
    const auto f32 = means.options(), i32 = means.options().dtype(at::kInt), i64 = means.options().dtype(at::kLong);
    auto outputs = [&](int64_t rows) {
        return std::make_tuple(at::empty({rows}, i64), at::empty({rows}, i64), at::empty({rows}, i64), at::zeros({B * C + 1}, i32),
                               at::empty({rows, 2}, i32), at::empty({rows, 2}, f32), at::empty({rows}, f32),
                               at::empty({rows, 3}, f32), calc_compensations ? OptTensor(at::empty({rows}, f32)) : OptTensor());
    };
    if (total == 0) return outputs(0); // nothing to launch (before the device is touched)
    Launch L(means_);
    auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(means.device().index());
    // rows are placed from BLOCK counts (csrc/projection.hip: PackedBlocks): one int32 per 256 pairs, scanned by one workgroup
    // that stores the row count straight into the pinned word below - no per-pair flags, no cumsum tensor, no copy kernel
    const int64_t n_blocks = gsx_project_packed_blocks(total);
    Tensor blocks = at::empty({2, n_blocks}, i32);
    Tensor host_nnz = at::empty({1}, at::TensorOptions().dtype(at::kLong).pinned_memory(true));
    volatile int64_t *nnz_slot = host_nnz.mutable_data_ptr<int64_t>();
    *nnz_slot = -1; // sentinel: the scan kernel overwrites it
    { Timed timed_("gsx_project_ewa_packed_count", L.stream); check(gsx_project_ewa_packed_count_blocks(fp(means), fp(covars), fp(quats), fp(scales), fp(opac), fp(viewmats), fp(Ks), (uint32_t)B,
                                       (uint32_t)C, (uint32_t)N, (uint32_t)width, (uint32_t)height, (float)eps2d,
                                       (float)near_plane, (float)far_plane, (float)radius_clip, (int)camera_model,
                                       calc_compensations ? 1 : 0, mp<int32_t>(blocks), mp<int32_t>(blocks) + n_blocks, nullptr,
                                       host_nnz.mutable_data_ptr<int64_t>(), L.stream),
          "gsx_project_ewa_packed_count_blocks"); }
    // The row count is on the host once the SCAN has run - the write kernel enqueued after it does not have to finish first:
    // the caller slices the outputs and enqueues the next kernels while the write kernel still runs (poll_host_word).
    auto wait_nnz = [&] { return poll_host_word(nnz_slot, [](int64_t v) { return v < 0; }, stream, std::chrono::seconds(2)); };
    auto write = [&](int64_t rows, decltype(outputs(0)) &o) {
        auto &[bi, ci, gi, indptr, radii, m2, dep, con, comp] = o;
        (void)rows;
        { Timed timed_("gsx_project_ewa_packed_write", L.stream); check(gsx_project_ewa_packed_write_blocks(fp(means), fp(covars), fp(quats), fp(scales), fp(opac), fp(viewmats), fp(Ks), (uint32_t)B,
                                           (uint32_t)C, (uint32_t)N, (uint32_t)width, (uint32_t)height, (float)eps2d,
                                           (float)near_plane, (float)far_plane, (float)radius_clip, (int)camera_model,
                                           cp<int32_t>(blocks) + n_blocks, mp<int64_t>(bi), mp<int64_t>(ci), mp<int64_t>(gi),
                                           mp<int32_t>(indptr), mp<int32_t>(radii), mp<float>(m2), mp<float>(dep), mp<float>(con),
                                           comp ? mp<float>(*comp) : nullptr, L.stream),
              "gsx_project_ewa_packed_write_blocks"); }
    };
    if (total * kPackedRowBytes <= kPackedPreallocLimit) {
        auto o = outputs(total);
        write(total, o);
        const int64_t nnz = wait_nnz(); // host round trip: exact-length COO outputs
        auto &[bi, ci, gi, indptr, radii, m2, dep, con, comp] = o;
        // a view pins the whole upper-bound buffer for as long as the step (and its autograd graph) holds the rows: copy the
        // heads out and let the big buffers go only when that is a real amount of memory (> 256 MiB) - the seven copies cost
        // 32 us of kernels and as much host time, which left the GPU idle behind the write pass (profiles/r08_ab.md #28)
        const bool compact = (total - nnz) * kPackedRowBytes > (int64_t(1) << 28);
        auto head = [&](const Tensor &t) { return compact ? t.narrow(0, 0, nnz).clone() : t.narrow(0, 0, nnz); };
        return {head(bi), head(ci), head(gi), indptr, head(radii), head(m2), head(dep), head(con),
                comp ? OptTensor(head(*comp)) : OptTensor()};
    }
    const int64_t nnz = wait_nnz();
    auto o = outputs(nnz);
    if (nnz > 0 || true) write(nnz, o);
    return o;
}
// ---- notes: what one op call leaves for a later one that the reference's op schemas have no slot for ------------------
// A note is keyed by the IDENTITY of a tensor, never by an address: a weak reference to its StorageImpl plus offset and
// length. The weak reference keeps that object's address from being handed out again for as long as the note exists, so a
// later tensor that the allocator placed at the same device address has another StorageImpl and does not match (keyed by
// data pointer, a call could pick up another intersection's value after allocator reuse, and which kernel ran - and so the
// float summation order - depended on the process' history).
struct TensorKey {
    std::optional<c10::weak_intrusive_ptr<c10::StorageImpl>> storage; // empty: no tensor
    int64_t offset = 0, n = 0;
    TensorKey() = default;
    explicit TensorKey(const Tensor &t)
    {
        if (!t.defined() || t.numel() <= 0 || !t.has_storage()) return;
        storage = c10::weak_intrusive_ptr<c10::StorageImpl>(
            c10::intrusive_ptr<c10::StorageImpl>::reclaim_copy(t.storage().unsafeGetStorageImpl()));
        offset = t.storage_offset(); n = t.numel();
    }
    const c10::StorageImpl *target() const { return storage ? storage->_unsafe_get_target() : nullptr; }
    bool expired() const { return storage && storage->expired(); }
    bool same_storage(const Tensor &t) const
    {
        return storage && t.defined() && t.has_storage() && target() == t.storage().unsafeGetStorageImpl();
    }
    bool matches(const Tensor &t) const { return same_storage(t) && offset == t.storage_offset() && n == t.numel(); }
};
// The slot a fresh note for `t` goes to: the one that holds t's storage already (noting again replaces), else a free one
// (never used, or its tensor has died), and only then the oldest.
static std::atomic<uint64_t> g_note_seq{0}; // orders the notes of a table by age
template <class Note, size_t N> Note &note_slot(Note (&table)[N], const Tensor &t)
{
    Note *pick = nullptr;
    for (auto &e : table)
        if (e.key.same_storage(t)) return e;
    for (auto &e : table)
        if (!e.key.storage || e.key.expired()) return e;
    for (auto &e : table)
        if (!pick || e.seq < pick->seq) pick = &e;
    return *pick;
}

// ---- longest tile list of an intersection result, for the compositing calls that consume it ---------------------------
// The fused intersection notes the longest list of the result it returns under the identity of `flatten_ids`; the
// compositing forward and backward look their `flatten_ids` up and cut long lists into segments above
// gsx_raster3d_seg_cut() (csrc/raster3d_seg.hip). This is the ONLY channel for that number, for rasterization() and for a
// caller that drives the stage ops itself (isect_tiles -> isect_offset_encode -> rasterize_to_pixels) alike. 0 = nothing
// noted: one workgroup per tile; a noted value below 0 says the same on purpose. A note that has not been consumed yet is
// lost only if 16 other intersections, whose flatten_ids are all still alive, are noted between an intersection and its
// compositing call: a fresh note takes a slot whose tensor has died before it takes the oldest.
struct LongestNote {
    TensorKey key;
    uint64_t seq = 0;
    int64_t longest = 0;
};
static std::mutex g_notes_mu;
static LongestNote g_notes[16];
void note_longest(const Tensor &flat, int64_t longest)
{
    TensorKey key(flat);
    if (!key.storage) return;
    std::lock_guard<std::mutex> lock(g_notes_mu);
    note_slot(g_notes, flat) = LongestNote{std::move(key), ++g_note_seq, longest};
}
int64_t lookup_longest(const Tensor &flat)
{
    std::lock_guard<std::mutex> lock(g_notes_mu);
    for (const auto &e : g_notes)
        if (e.key.matches(flat)) return e.longest;
    return 0;
}

// ---- the segment workspace of a compositing FORWARD, for the backward over the same lists ------------------------------
// gsx_raster3d_fwd_seg leaves every slice's colour sums and end transmittance in its workspace; a backward that still has it
// needs no pre-pass (gsx_raster3d_bwd_seg_reuse). The forward body notes it under the identity of the `last_ids` it returns
// (the tensor every autograd formula - this package's and the reference's own - saves and hands to the backward op). The
// workspace itself is held STRONGLY (tens of MB for a 1080p scene) in a table of four; a note whose last_ids died is
// dropped at the next call of either function.
// The sums in the workspace belong to the forward's INPUTS: a backward call that brings other tensors than the forward saw
// (identity), or the same ones written to since (version counter), gets no workspace and runs its pre-pass on what it was
// given.
struct SegWsNote {
    TensorKey key;
    uint64_t seq = 0;
    int64_t n_isects = 0, cdim = 0, seg_len = 0;
    std::vector<std::pair<TensorKey, int64_t>> inputs; // (identity, version) of every tensor the forward composited from
    Tensor ws;
    bool made_from(at::TensorList ts) const
    {
        if (ts.size() != inputs.size()) return false;
        for (size_t i = 0; i < inputs.size(); ++i)
            if (!inputs[i].first.matches(ts[i]) || inputs[i].second != tensor_version(ts[i])) return false;
        return true;
    }
    static int64_t tensor_version(const Tensor &t) { return t.defined() && !t.is_inference() ? (int64_t)t._version() : 0; }
};
static std::mutex g_seg_ws_mu;
static SegWsNote g_seg_ws[4];
static void seg_ws_purge_locked()
{
    for (auto &e : g_seg_ws)
        if (e.key.expired()) e = SegWsNote();
}
void note_seg_workspace(const Tensor &last_ids, const Tensor &ws, int64_t n_isects, int64_t cdim, int64_t seg_len,
                        at::TensorList inputs)
{
    SegWsNote fresh;
    fresh.key = TensorKey(last_ids);
    if (!fresh.key.storage) return;
    fresh.n_isects = n_isects; fresh.cdim = cdim; fresh.seg_len = seg_len; fresh.ws = ws;
    for (const Tensor &t : inputs) fresh.inputs.emplace_back(TensorKey(t), SegWsNote::tensor_version(t));
    std::lock_guard<std::mutex> lock(g_seg_ws_mu);
    seg_ws_purge_locked();
    fresh.seq = ++g_note_seq;
    note_slot(g_seg_ws, last_ids) = std::move(fresh);
}
OptTensor lookup_seg_workspace(const Tensor &last_ids, int64_t n_isects, int64_t cdim, int64_t seg_len, at::TensorList inputs)
{
    std::lock_guard<std::mutex> lock(g_seg_ws_mu);
    seg_ws_purge_locked();
    for (const auto &e : g_seg_ws)
        if (e.key.matches(last_ids) && e.made_from(inputs) && e.n_isects == n_isects && e.cdim == cdim && e.seg_len == seg_len
            && e.ws.defined() && e.ws.device() == last_ids.device())
            return e.ws;
    return std::nullopt;
}
static bool seg_reuse_env()
{
    static const bool v = [] {
        const char *e = std::getenv("GSPLAT_AMD_SEG_REUSE"); // 0: always the pre-pass (A/B)
        return !(e && (e[0] == '0' || e[0] == 0));
    }();
    return v;
}

// ---- tile intersection --------------------------------------------------------------------------------------------------
Tensor bytes(int64_t n, const Tensor &like) { return at::empty({n < 8 ? 8 : n}, like.options().dtype(at::kByte)); }

Tensor intersect_offset(const Tensor &isect_ids_, int64_t I, int64_t tile_w, int64_t tile_h)
{
    Launch L(isect_ids_);
    const Tensor ids = contig(isect_ids_);
    Tensor offsets = at::empty({I, tile_h, tile_w}, ids.options().dtype(at::kInt));
    { Timed timed_("gsx_isect_offsets", L.stream); check(gsx_isect_offsets(cp<int64_t>(ids), ids.numel(), (uint32_t)I, (uint32_t)tile_w, (uint32_t)tile_h, mp<int32_t>(offsets),
                            L.stream),
          "gsx_isect_offsets"); }
    return offsets;
}

// ---- compositing --------------------------------------------------------------------------------------------------------
struct RasterDims {
    std::vector<int64_t> image_dims;
    int64_t I, th, tw, D;
};
RasterDims raster_dims(const Tensor &isect_offsets, const Tensor &colors)
{
    RasterDims r;
    r.image_dims.assign(isect_offsets.sizes().begin(), isect_offsets.sizes().end() - 2);
    r.I = prod(r.image_dims);
    r.th = isect_offsets.size(-2);
    r.tw = isect_offsets.size(-1);
    r.D = colors.size(-1);
    return r;
}

// segment length / the longest list from which segmenting starts; GSPLAT_AMD_SEG_LEN overrides (A/B), 0 switches it off
static int64_t seg_len_env()
{
    static const int64_t v = [] {
        const char *e = std::getenv("GSPLAT_AMD_SEG_LEN");
        return e ? (int64_t)std::atoll(e) : (int64_t)768;
    }();
    return v;
}
#define kSegLen (seg_len_env())

std::tuple<Tensor, Tensor, Tensor, Tensor>
rasterize_to_pixels_3dgs(const Tensor &means2d_, const Tensor &conics_, const Tensor &colors_, const Tensor &opacities_,
                         const OptTensor &backgrounds_, const OptTensor &masks_, int64_t width, int64_t height, int64_t tile_size,
                         const Tensor &isect_offsets_, const Tensor &flatten_ids_, bool packed, bool absgrad)
{
    (void)packed;
    want_f32(means2d_, "means2d"); want_f32(conics_, "conics"); want_f32(colors_, "colors"); want_f32(opacities_, "opacities");
    want_f32(backgrounds_, "backgrounds");
    Launch L(means2d_);
    const RasterDims r = raster_dims(isect_offsets_, colors_);
    TORCH_CHECK(r.th * tile_size >= height && r.tw * tile_size >= width,
                      "rasterize_to_pixels: isect_offsets tile grid does not cover the image");
    TORCH_CHECK(!has(masks_) || masks_->scalar_type() == at::kBool, "masks must be a bool tensor");
    const Tensor means2d = contig(means2d_), conics = contig(conics_), colors = contig(colors_), opac = contig(opacities_);
    const OptTensor bg = contig(backgrounds_), masks = contig(masks_);
    const Tensor offsets = contig(isect_offsets_), flat = contig(flatten_ids_);
    auto shape = [&](std::initializer_list<int64_t> tail) {
        auto s = r.image_dims;
        s.insert(s.end(), tail);
        return s;
    };
    Tensor renders = at::empty(shape({height, width, r.D}), means2d.options());
    Tensor alphas = at::empty(shape({height, width, 1}), means2d.options());
    Tensor last_ids = at::empty(shape({height, width}), means2d.options().dtype(at::kInt));
    const int64_t longest = lookup_longest(flatten_ids_); // what the intersection that made these lists noted
    if (kSegLen > 0 && longest > gsx_raster3d_seg_cut(flat.numel(), (uint32_t)r.I, (uint32_t)r.tw, (uint32_t)r.th, (uint32_t)kSegLen)) {
        Tensor ws = at::empty({gsx_raster3d_seg_workspace_bytes(flat.numel(), (uint32_t)r.I, (uint32_t)r.tw, (uint32_t)r.th, (uint32_t)r.D,
                                                              (uint32_t)kSegLen)}, means2d.options().dtype(at::kByte));
        Timed timed_("gsx_raster3d_fwd", L.stream); // same stage name: it IS the compositing forward
        check(gsx_raster3d_fwd_seg(fp(means2d), fp(conics), fp(colors), fp(opac), fp(bg),
                                   masks ? (const uint8_t *)masks->const_data_ptr<bool>() : nullptr, cp<int32_t>(offsets),
                                   cp<int32_t>(flat), (uint32_t)r.I, (uint32_t)flat.numel(), (uint32_t)r.D, (uint32_t)width,
                                   (uint32_t)height, (uint32_t)tile_size, (uint32_t)r.tw, (uint32_t)r.th, mp<float>(renders),
                                   mp<float>(alphas), mp<int32_t>(last_ids), (uint32_t)kSegLen, ws.mutable_data_ptr(), ws.numel(), L.stream),
              "gsx_raster3d_fwd_seg");
        // the backward over these lists starts its slices from the sums this call left (no pre-pass): <= 4 channels only
        if (r.D <= 4 && tile_size == 16 && seg_reuse_env())
            note_seg_workspace(last_ids, ws, flat.numel(), r.D, kSegLen, {means2d_, conics_, colors_, opacities_, isect_offsets_, flatten_ids_});
    } else { Timed timed_("gsx_raster3d_fwd", L.stream); check(gsx_raster3d_fwd(fp(means2d), fp(conics), fp(colors), fp(opac), fp(bg),
                           masks ? (const uint8_t *)masks->const_data_ptr<bool>() : nullptr, cp<int32_t>(offsets),
                           cp<int32_t>(flat), (uint32_t)r.I, (uint32_t)flat.numel(), (uint32_t)r.D, (uint32_t)width,
                           (uint32_t)height, (uint32_t)tile_size, (uint32_t)r.tw, (uint32_t)r.th, mp<float>(renders),
                           mp<float>(alphas), mp<int32_t>(last_ids), L.stream),
          "gsx_raster3d_fwd"); }
    Tensor holder = absgrad ? at::zeros_like(means2d) : at::empty({0}, means2d.options());
    return {renders, alphas, holder, last_ids};
}

// ---- the two halves of the fused intersection (gsplat_amd/_ops.py: isect_begin / isect_finish, behind intersect_tile) ------
// The orchestrators (rendering.py) enqueue the SH kernels between the halves instead of blocking on the intersection count;
// private ops (namespace gsplat_amd: not part of the reference's surface). The count travels through a pinned host word initialised to a
// sentinel: the second half polls it - no event, no stream synchronisation, and the kernels enqueued in between keep running.
// This is the one place where the host protocol of the fused intersection lives (decide the path once, count, wait, count
// again Gaussian-major on GSX_ISECT_RETRY, emit): the sparse intersection comes through here too, with its `tile_mask` (only
// flagged tiles receive intersections) and an empty `out_shape` (= no tiles_per_gauss wanted).
const uint8_t *mask_ptr(const OptTensor &m) { return has(m) && m->numel() ? (const uint8_t *)m->const_data_ptr<bool>() : nullptr; }

std::tuple<OptTensor, Tensor, Tensor, Tensor>
isect_fused_begin(const Tensor &means2d, const Tensor &radii, const Tensor &depths, const OptTensor &conics, const OptTensor &opac,
                  const OptTensor &tile_mask, int64_t rows, int64_t I, int64_t tile_size, int64_t tile_w, int64_t tile_h, c10::IntArrayRef out_shape)
{
    Launch L(means2d);
    const uint32_t uI = (uint32_t)I, uts = (uint32_t)tile_size, utw = (uint32_t)tile_w, uth = (uint32_t)tile_h;
    TORCH_CHECK(!has(tile_mask) || (tile_mask->scalar_type() == at::kBool && tile_mask->is_contiguous()
                                    && tile_mask->numel() == I * tile_w * tile_h),
                "isect_fused_begin: tile_mask must be a contiguous bool tensor of n_images * tiles flags");
    Tensor tiles_per_gauss; // stays undefined (a null pointer for the kernels, None for the caller) when none is wanted
    if (!out_shape.empty()) tiles_per_gauss = at::empty(out_shape, means2d.options().dtype(at::kInt));
    auto result = [&](const Tensor &offsets, const Tensor &count_ws, const Tensor &host_total) {
        return std::make_tuple(tiles_per_gauss.defined() ? OptTensor(tiles_per_gauss) : OptTensor(), offsets, count_ws, host_total);
    };
    // pinned host words: [0] n_isects (sentinel -1 until the count has run), [1] the longest tile list (written first)
    // [2] which count ran (1 = tile-owner-major): the second half reads the workspace laid out by THIS choice, whatever the
    // environment switches say by then
    Tensor host_total = at::empty({3}, at::TensorOptions().dtype(at::kLong).pinned_memory(true));
    host_total.mutable_data_ptr<int64_t>()[0] = -1;
    host_total.mutable_data_ptr<int64_t>()[1] = 0;
    const bool binned_path = gsx_isect_binned_should_try(rows, uI, utw, uth, 0) != 0; // the one decision; slot [2] carries it
    host_total.mutable_data_ptr<int64_t>()[2] = binned_path ? 1 : 0;
    Tensor offsets = at::empty({I * tile_w * tile_h}, means2d.options().dtype(at::kInt));
    if (binned_path) { // tile-owner-major path (csrc/isect_binned.hip)
        Tensor count_ws = bytes(gsx_isect_binned_count_workspace_bytes(rows, uI, utw, uth), means2d);
        { Timed timed_("gsx_isect_binned_count", L.stream); check(gsx_isect_binned_count(fp(means2d), cp<int32_t>(radii), fp(depths), fp(conics), fp(opac), mask_ptr(tile_mask), rows, uI, uts,
                                     utw, uth, mp<int32_t>(tiles_per_gauss), mp<int32_t>(offsets), host_total.mutable_data_ptr<int64_t>(),
                                     host_total.mutable_data_ptr<int64_t>() + 1, count_ws.mutable_data_ptr(), count_ws.numel(), L.stream),
              "gsx_isect_binned_count"); }
        return result(offsets, count_ws, host_total);
    }
    Tensor count_ws = bytes(gsx_isect_fused_count_workspace_bytes(rows, uI, utw, uth), means2d);
    { Timed timed_("gsx_isect_fused_count", L.stream); check(gsx_isect_fused_count(fp(means2d), cp<int32_t>(radii), fp(conics), fp(opac), mask_ptr(tile_mask), rows, uI, uts, utw, uth,
                                mp<int32_t>(tiles_per_gauss), mp<int32_t>(offsets), host_total.mutable_data_ptr<int64_t>(),
                                host_total.mutable_data_ptr<int64_t>() + 1, count_ws.mutable_data_ptr(), count_ws.numel(), L.stream),
          "gsx_isect_fused_count"); }
    return result(offsets, count_ws, host_total);
}

std::tuple<Tensor, Tensor>
isect_fused_finish(const Tensor &means2d, const Tensor &radii, const Tensor &depths, const OptTensor &conics, const OptTensor &opac,
                   const OptTensor &tile_mask, int64_t rows, int64_t I, int64_t tile_size, int64_t tile_w, int64_t tile_h, Tensor count_ws,
                   const Tensor &offsets, const Tensor &host_total, const OptTensor &tiles_per_gauss_)
{
    Tensor tiles_per_gauss = has(tiles_per_gauss_) ? *tiles_per_gauss_ : Tensor();
    Launch L(means2d);
    const uint32_t uI = (uint32_t)I, uts = (uint32_t)tile_size, utw = (uint32_t)tile_w, uth = (uint32_t)tile_h;
    volatile const int64_t *slot = host_total.const_data_ptr<int64_t>();
    auto hip_stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(means2d.device().index());
    int64_t M = poll_host_word(slot, [](int64_t v) { return v == -1; }, hip_stream, std::chrono::seconds(5));
    TORCH_CHECK(host_total.numel() > 2, "isect_fused_finish: host_total must be the three pinned words of isect_fused_begin");
    bool binned = slot[2] != 0; // the choice isect_fused_begin made (never re-derived: a query here could answer differently)
    if (binned && M == GSX_ISECT_RETRY) {
        // the binned path's entry workspace was too small for this scene (very large Gaussians), or a bin too crowded: count
        // again Gaussian-major, and do not try this shape again for a while
        binned   = false;
        gsx_isect_binned_note_retry(rows, uI, utw, uth);
        count_ws = bytes(gsx_isect_fused_count_workspace_bytes(rows, uI, utw, uth), means2d);
        { Timed timed_("gsx_isect_fused_count", L.stream); check(gsx_isect_fused_count(fp(means2d), cp<int32_t>(radii), fp(conics), fp(opac), mask_ptr(tile_mask), rows, uI, uts, utw, uth,
                                    mp<int32_t>(tiles_per_gauss), offsets.mutable_data_ptr<int32_t>(),
                                    host_total.mutable_data_ptr<int64_t>(), host_total.mutable_data_ptr<int64_t>() + 1,
                                    count_ws.mutable_data_ptr(), count_ws.numel(), L.stream),
              "gsx_isect_fused_count"); }
        hip_stream.synchronize();
        M = *slot;
    }
    TORCH_CHECK(M >= 0, "intersect_tile: the intersection count never reached the host");
    TORCH_CHECK(M < (1ll << 31), "intersect_tile: ", M, " intersections overflow the int32 index space");
    Tensor ids = at::empty({M}, means2d.options().dtype(at::kLong)), flat = at::empty({M}, means2d.options().dtype(at::kInt));
    if (M == 0) return {ids, flat};
    if (binned) {
        Tensor ws = bytes(gsx_isect_binned_emit_workspace_bytes(M), means2d);
        { Timed timed_("gsx_isect_binned_emit_sort", L.stream); check(gsx_isect_binned_emit_sort(rows, uI, uts, utw, uth, count_ws.mutable_data_ptr(), count_ws.numel(),
                                         cp<int32_t>(offsets), M, (int64_t)slot[1], mp<int64_t>(ids), mp<int32_t>(flat), ws.mutable_data_ptr(), ws.numel(), L.stream),
              "gsx_isect_binned_emit_sort"); }
        note_longest(flat, (int64_t)slot[1]);
        return {ids, flat};
    }
    Tensor ws = bytes(gsx_isect_fused_emit_workspace_bytes(M, uI, utw, uth), means2d);
    { Timed timed_("gsx_isect_fused_emit_sort", L.stream); check(gsx_isect_fused_emit_sort(fp(means2d), cp<int32_t>(radii), fp(depths), fp(conics), fp(opac), mask_ptr(tile_mask), rows, uI, uts,
                                    utw, uth, count_ws.mutable_data_ptr(), count_ws.numel(), cp<int32_t>(offsets), M,
                                    mp<int64_t>(ids), mp<int32_t>(flat), ws.mutable_data_ptr(), ws.numel(), L.stream),
          "gsx_isect_fused_emit_sort"); }
    note_longest(flat, (int64_t)slot[1]);
    return {ids, flat};
}

// ---- 2DGS: the two forward ops on the critical host path of rasterization_2dgs ----------------------------------------------
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor>
projection_2dgs_fused(const Tensor &means_, const Tensor &quats_, const Tensor &scales_, const Tensor &viewmats_, const Tensor &Ks_,
                      int64_t width, int64_t height, double eps2d, double near_plane, double far_plane, double radius_clip)
{
    (void)eps2d; // accepted and unused, as in the reference (Projection2DGSFused.cu evaluates the box at one sigma)
    want_f32(means_, "means"); want_f32(quats_, "quats"); want_f32(scales_, "scales"); want_f32(viewmats_, "viewmats");
    want_f32(Ks_, "Ks");
    const int64_t N = means_.size(-2);
    TORCH_CHECK(means_.size(-1) == 3 && quats_.dim() >= 2 && quats_.size(-2) == N && quats_.size(-1) == 4
                          && scales_.dim() >= 2 && scales_.size(-2) == N && scales_.size(-1) == 3,
                      "projection_2dgs: bad shapes means ", means_.sizes(), " quats ", quats_.sizes(), " scales ", scales_.sizes());
    const Tensor means = contig(means_), quats = contig(quats_), scales = contig(scales_), viewmats = contig(viewmats_),
                 Ks = contig(Ks_);
    const int64_t B = prod(means.sizes().slice(0, means.dim() - 2)), C = viewmats.size(-3);
    std::vector<int64_t> shape(means.sizes().begin(), means.sizes().end() - 2);
    shape.push_back(C); shape.push_back(N);
    auto with = [&](std::initializer_list<int64_t> tail) {
        auto s = shape;
        s.insert(s.end(), tail);
        return s;
    };
    Tensor radii = at::empty(with({2}), means.options().dtype(at::kInt)), means2d = at::empty(with({2}), means.options());
    Tensor depths = at::empty(shape, means.options()), rt = at::empty(with({3, 3}), means.options());
    Tensor normals = at::empty(with({3}), means.options());
    if (B * C * N == 0) return {radii, means2d, depths, rt, normals}; // nothing to launch (before the device is touched)
    Launch L(means_);
    { Timed timed_("gsx_project_2dgs_fwd", L.stream); check(gsx_project_2dgs_fwd(fp(means), fp(quats), fp(scales), fp(viewmats), fp(Ks), (uint32_t)B, (uint32_t)C, (uint32_t)N,
                               (uint32_t)width, (uint32_t)height, (float)near_plane, (float)far_plane, (float)radius_clip,
                               mp<int32_t>(radii), mp<float>(means2d), mp<float>(depths), mp<float>(rt), mp<float>(normals),
                               L.stream),
          "gsx_project_2dgs_fwd"); }
    return {radii, means2d, depths, rt, normals};
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>
rasterize_to_pixels_2dgs(const Tensor &means2d_, const Tensor &ray_transforms_, const Tensor &colors_, const Tensor &opacities_,
                         const Tensor &normals_, const Tensor &densify, const OptTensor &backgrounds_, const OptTensor &masks_,
                         int64_t width, int64_t height, int64_t tile_size, const Tensor &tile_offsets_, const Tensor &flatten_ids_,
                         bool packed, bool absgrad, bool distloss)
{
    (void)packed; (void)densify;
    want_f32(means2d_, "means2d"); want_f32(ray_transforms_, "ray_transforms"); want_f32(colors_, "colors");
    want_f32(opacities_, "opacities"); want_f32(normals_, "normals"); want_f32(backgrounds_, "backgrounds");
    Launch L(means2d_);
    const RasterDims r = raster_dims(tile_offsets_, colors_);
    TORCH_CHECK(r.th * tile_size >= height && r.tw * tile_size >= width,
                      "rasterize_to_pixels_2dgs: tile grid does not cover the image");
    TORCH_CHECK(!has(masks_) || masks_->scalar_type() == at::kBool, "masks must be a bool tensor");
    const Tensor means2d = contig(means2d_), rt = contig(ray_transforms_), colors = contig(colors_), opac = contig(opacities_),
                 normals = contig(normals_);
    const OptTensor bg = contig(backgrounds_), masks = contig(masks_);
    const Tensor offsets = contig(tile_offsets_), flat = contig(flatten_ids_);
    auto shape = [&](std::initializer_list<int64_t> tail) {
        auto s = r.image_dims;
        s.insert(s.end(), tail);
        return s;
    };
    const auto f32 = means2d.options(), i32 = means2d.options().dtype(at::kInt);
    Tensor renders = at::empty(shape({height, width, r.D}), f32), alphas = at::empty(shape({height, width, 1}), f32);
    Tensor rnormals = at::empty(shape({height, width, 3}), f32), rdistort = at::empty(shape({height, width, 1}), f32);
    Tensor rmedian = at::empty(shape({height, width, 1}), f32);
    Tensor last_ids = at::empty(shape({height, width}), i32), median_ids = at::empty(shape({height, width}), i32);
    { Timed timed_("gsx_raster2d_fwd", L.stream); check(gsx_raster2d_fwd(fp(means2d), fp(rt), fp(colors), fp(opac), fp(normals), fp(bg),
                           masks ? (const uint8_t *)masks->const_data_ptr<bool>() : nullptr, cp<int32_t>(offsets),
                           cp<int32_t>(flat), (uint32_t)r.I, (uint32_t)flat.numel(), (uint32_t)r.D, (uint32_t)width,
                           (uint32_t)height, (uint32_t)tile_size, (uint32_t)r.tw, (uint32_t)r.th, distloss ? 1 : 0,
                           mp<float>(renders), mp<float>(alphas), mp<float>(rnormals), mp<float>(rdistort), mp<float>(rmedian),
                           mp<int32_t>(last_ids), mp<int32_t>(median_ids), L.stream),
          "gsx_raster2d_fwd"); }
    Tensor holder = absgrad ? at::zeros_like(means2d) : at::empty({0}, f32);
    return {renders, alphas, rnormals, rdistort, rmedian, holder, last_ids, median_ids};
}

} // namespace
} // namespace gsplat_amd

// gsplat_amd/_ops.py (ctypes): the segment length the compiled compositing forward uses, for the Python backward body
extern "C" int64_t gsx_torch_seg_len() { return gsplat_amd::seg_len_env(); }

TORCH_LIBRARY(gsplat_amd, m)
{
    m.def("isect_fused_begin(Tensor means2d, Tensor radii, Tensor depths, Tensor? conics, Tensor? opacities, Tensor? tile_mask, int rows, int n_images, int tile_size, "
          "int tile_w, int tile_h, int[] out_shape) -> (Tensor?, Tensor, Tensor, Tensor)");
    m.def("isect_fused_finish(Tensor means2d, Tensor radii, Tensor depths, Tensor? conics, Tensor? opacities, Tensor? tile_mask, int rows, int n_images, "
          "int tile_size, int tile_w, int tile_h, Tensor count_ws, Tensor offsets, Tensor host_total, Tensor? tiles_per_gauss) -> (Tensor, Tensor)");
    // the notes, for the Python op bodies (the compositing backward looks up the longest list and the forward's segment
    // workspace) and for tests
    m.def("note_longest(Tensor flatten_ids, int longest) -> ()");
    m.def("lookup_longest(Tensor flatten_ids) -> int");
    m.def("lookup_seg_workspace(Tensor last_ids, int n_isects, int cdim, int seg_len, Tensor[] inputs) -> Tensor?");
}

TORCH_LIBRARY_IMPL(gsplat_amd, CUDA, m)
{
    m.impl("isect_fused_begin", &gsplat_amd::isect_fused_begin);
    m.impl("isect_fused_finish", &gsplat_amd::isect_fused_finish);
}

// the notes are keyed by storage identity: any backend (tools/dry_run.py drives the host paths with CPU tensors)
TORCH_LIBRARY_IMPL(gsplat_amd, CompositeExplicitAutograd, m)
{
    m.impl("note_longest", &gsplat_amd::note_longest);
    m.impl("lookup_longest", &gsplat_amd::lookup_longest);
    m.impl("lookup_seg_workspace", &gsplat_amd::lookup_seg_workspace);
}

TORCH_LIBRARY_IMPL(gsplat, CUDA, m)
{
    using namespace gsplat_amd;
    m.impl("projection_ewa_3dgs_fused", &projection_ewa_3dgs_fused);
    m.impl("projection_ewa_3dgs_packed", &projection_ewa_3dgs_packed);
    m.impl("intersect_offset", &intersect_offset);
    m.impl("rasterize_to_pixels_3dgs", &rasterize_to_pixels_3dgs);
    m.impl("projection_2dgs_fused", &projection_2dgs_fused);
    m.impl("rasterize_to_pixels_2dgs", &rasterize_to_pixels_2dgs);
}

// timing hooks for gsplat_amd/_cabi.py: begin(only = space-separated entry points or "" for all); end() returns
// "name ms\n" per timed call (synchronises the events) in a buffer owned by this library until the next call
extern "C" void gsx_torch_profile_begin(const char *only)
{
    using namespace gsplat_amd;
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    g_prof_only.clear();
    std::string w;
    for (const char *p = only ? only : ""; ; ++p) {
        if (*p == ' ' || *p == 0) {
            if (!w.empty()) g_prof_only.insert(w);
            w.clear();
            if (*p == 0) break;
        } else w.push_back(*p);
    }
    g_prof_on = true;
}

extern "C" const char *gsx_torch_profile_end()
{
    using namespace gsplat_amd;
    static std::string out;
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    g_prof_on = false;
    out.clear();
    for (auto &r : g_prof) {
        float ms = 0.0f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess)
            out += r.name + " " + std::to_string(ms) + "\n";
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    g_prof.clear();
    return out.c_str();
}
