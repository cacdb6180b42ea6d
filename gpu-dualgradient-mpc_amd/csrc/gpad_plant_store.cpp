// gpad_plant_store.cpp -- PlantStore (gpad_plant_store.h): layout, validation, upload and packing of the plant
// maps and signal images.  Arrays are numbered PM, M0, Pg, g0, A, B = 0 .. 5 throughout.
#include <algorithm>

#include "gpad_host.h"

namespace gpad {
namespace {

struct Layout {
    size_t elems[6];  // of one copy of each array
    size_t off[6];    // element offset of each array, `copies` consecutive copies long
    size_t total;
};

Layout lay_out(const size_t (&elems)[6], size_t copies) {
    Layout l{};
    for (int i = 0; i < 6; ++i) {
        l.elems[i] = elems[i];
        l.off[i] = l.total;
        l.total += copies * elems[i];
    }
    return l;
}

// the six maps
Layout map_layout(const PlantStore& p, size_t copies) {
    const size_t n = p.n, m = p.m, nx = p.nx, nu = p.nu;
    return lay_out({n * nx, n, m * nx, m, nx * nx, nx * nu}, copies);
}

// the packed images in the places of PM, Pg, A (rows of nx + ns columns) and, replicated: M0, g0, B in theirs
Layout image_layout(const PlantStore& p, int ns, size_t copies, bool replicated) {
    const size_t n = p.n, m = p.m, nx = p.nx, w = nx + ns, r = replicated ? 1 : 0;
    return lay_out({n * w, r * n, m * w, r * m, nx * w, r * nx * p.nu}, copies);
}

}  // namespace

int PlantStore::bind_plant(const char* fn, const gpad_dims_t& d, int stack, int nx_, int nu_, const void* PM,
                           const void* M0, const void* Pg, const void* g0, const void* A, const void* B,
                           hipStream_t s) {
    const std::string where(fn);
    if (nx_ <= 0 || nu_ < 0 || !PM || !Pg) return fail(GPAD_ERR_INVALID, where + ": bad arguments");
    if ((A == nullptr) != (B == nullptr) || (A && nu_ == 0))
        return fail(GPAD_ERR_INVALID, where + ": give A and B together (nu >= 1)");
    if (nu_ > d.n) return fail(GPAD_ERR_INVALID, where + ": nu > n");
    unbind();
    n = d.n;
    m = d.m;
    dtype = d.dtype;
    nx = nx_;
    nu = nu_;
    const int ncopies = stack ? stack : 1;
    const Layout l = map_layout(*this, (size_t)ncopies);
    const size_t es = esize(dtype);
    if (int rc = maps.ensure(es * l.total)) return rc;
    const hipMemcpyKind kind = d.memory == GPAD_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const void* src[6] = {PM, M0, Pg, g0, A, B};
    for (int i = 0; i < 6; ++i)
        if (src[i] && l.elems[i])
            HIP_TRY(hipMemcpyAsync((char*)maps.p + es * l.off[i], src[i], es * ncopies * l.elems[i], kind, s));
    HIP_TRY(hipStreamSynchronize(s));
    has_M0 = M0 != nullptr;
    has_g0 = g0 != nullptr;
    dyn = A != nullptr;
    copies = ncopies;
    stacked = stack > 0;
    return GPAD_OK;
}

// stages host maps in *up, packs the three images and replicates M0, g0, B where the plant has one copy under
// `ncopies` > 1 signal copies
template <typename T>
int PlantStore::pack(int memory, int ns_, int ncopies, const T* const S_in[3], DevBuf* up, hipStream_t s) {
    const size_t ic = (size_t)std::max(copies, ncopies);
    const bool replicated = (size_t)copies < ic;
    const Layout lm = map_layout(*this, (size_t)copies), li = image_layout(*this, ns_, ic, replicated);
    if (int rc = images.ensure(sizeof(T) * li.total)) return rc;
    const size_t rows[3] = {(size_t)n, (size_t)m, dyn ? (size_t)nx : 0};
    const T* S[3] = {S_in[0], S_in[1], S_in[2]};
    if (memory == GPAD_MEM_HOST) {
        size_t total = 0, off = 0;
        for (int i = 0; i < 3; ++i) total += S[i] ? ncopies * rows[i] * ns_ : 0;
        if (int rc = up->ensure(sizeof(T) * total)) return rc;
        for (int i = 0; i < 3; ++i) {
            const size_t elems = ncopies * rows[i] * ns_;
            if (!S[i] || !elems) continue;
            HIP_TRY(hipMemcpyAsync((T*)up->p + off, S[i], sizeof(T) * elems, hipMemcpyHostToDevice, s));
            S[i] = (const T*)up->p + off;
            off += elems;
        }
    }
    const T* P = (const T*)maps.p;
    T* I = (T*)images.p;
    for (int i = 0; i < 3; ++i) {
        const int a = 2 * i;  // PM, Pg, A
        if (!rows[i]) continue;
        if (copies == ncopies) {  // copy k of the plant with copy k of the signals: the arrays are contiguous
            HIP_TRY(launch_pack_aug<T>(P + lm.off[a], S[i], I + li.off[a], (long long)(ic * rows[i]), nx, ns_, s));
            continue;
        }
        for (size_t k = 0; k < ic; ++k)  // (the side with one copy lends it to every k)
            HIP_TRY(launch_pack_aug<T>(P + lm.off[a] + (copies > 1 ? k : 0) * lm.elems[a],
                                       S[i] ? S[i] + (ncopies > 1 ? k : 0) * rows[i] * ns_ : nullptr,
                                       I + li.off[a] + k * li.elems[a], (long long)rows[i], nx, ns_, s));
    }
    const bool given[6] = {true, has_M0, true, has_g0, dyn, dyn};
    for (int a = 1; a < 6 && replicated; a += 2)  // M0, g0, B
        for (size_t k = 0; k < ic && given[a] && li.elems[a]; ++k)
            HIP_TRY(hipMemcpyAsync(I + li.off[a] + k * li.elems[a], P + lm.off[a], sizeof(T) * li.elems[a],
                                   hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GPAD_OK;
}

int PlantStore::bind_signals(int memory, int ns_, int stack, const void* SM, const void* Sg, const void* E,
                             hipStream_t s) {
    ns = 0;
    if (ns_ == 0) return GPAD_OK;
    const int ncopies = stack ? stack : 1;
    DevBuf up;
    int rc;
    if (dtype == GPAD_DTYPE_F64) {
        const double* S[3] = {(const double*)SM, (const double*)Sg, (const double*)E};
        rc = pack<double>(memory, ns_, ncopies, S, &up, s);
    } else {
        const float* S[3] = {(const float*)SM, (const float*)Sg, (const float*)E};
        rc = pack<float>(memory, ns_, ncopies, S, &up, s);
    }
    up.release();
    if (rc) return rc;
    ns = ns_;
    sig_copies = ncopies;
    sig_stacked = stack > 0;
    return GPAD_OK;
}

template <typename T>
PlantView<T> PlantStore::view(int first, bool all, bool with_sig) const {
    const int sn = with_sig ? ns : 0;
    const size_t c = (size_t)(sn ? image_copies() : copies), k = all ? 0 : (size_t)first;
    const bool replicated = sn && (size_t)copies < c;
    const Layout lm = map_layout(*this, (size_t)copies), li = image_layout(*this, sn, c, replicated);
    auto at = [&](int a) -> const T* {  // array a of copy k; a holder of one copy lends it to every k
        const bool image = sn && (a % 2 == 0 || replicated);
        const Layout& l = image ? li : lm;
        return (const T*)(image ? images.p : maps.p) + l.off[a] + ((image ? c : (size_t)copies) > 1 ? k : 0) * l.elems[a];
    };
    PlantView<T> v{};
    v.PM = at(0);
    v.M0 = has_M0 ? at(1) : nullptr;
    v.Pg = at(2);
    v.g0 = has_g0 ? at(3) : nullptr;
    v.A = at(4);
    v.B = at(5);
    v.nxa = nx + sn;
    v.copies = (int)c;
    v.per_copy = all && (stacked || (sn && sig_stacked));
    return v;
}
template PlantView<float> PlantStore::view<float>(int, bool, bool) const;
template PlantView<double> PlantStore::view<double>(int, bool, bool) const;

}  // namespace gpad
