// net.h -- extractor-network interface behind kpb_net_*, the .kpbw weight container parser, and what the nets share with the LightGlue matcher.
#pragma once
#include "kpb_common.h"

#include <map>
#include <memory>
#include <stdexcept>

struct kpb_net {
    kpb_ctx* ctx = nullptr;
    int arch = 0;
    int dim = 0;        // descriptor channels
    int desc_div = 1;   // descriptor map is (H/desc_div) x (W/desc_div)
    float* wdev = nullptr;                 // all repacked weights: every network keeps typed pointers into it, bound once at create (WeightStage::put)
    kpb_buf act;                           // activations of the last forward, carved by kpb_carve
    int B = 0, H = 0, W = 0;
    virtual ~kpb_net() { (void)hipFree(wdev); (void)hipFree(act.p); }      // on the context's device: kpb_net_destroy, or a create that failed part way
    virtual int forward(const float* img, int batch, int H, int W, float* score_out, float* desc_out) = 0;
    virtual int desc_at(const float* pts, int pts_cols, int max_n, const int32_t* n_dev, float* out)
    {
        (void)pts; (void)pts_cols; (void)max_n; (void)n_dev; (void)out;
        return kpb_fail(ctx, KPB_E_INVALID, "kpb_net_desc_at: this network materialises its descriptor map; use kpb_sample");
    }
};

// a create's refusal of a weight blob (KpbwReader::need): what() is the whole message, guarded() answers KPB_E_WEIGHTS with it
struct KpbwMissing : std::runtime_error { using std::runtime_error::runtime_error; };

// runs network and matcher code behind the C API: no C++ exception may cross it
template <class F> int guarded(kpb_ctx* ctx, const char* what, F&& f)
{
    try { return f(); }
    catch (const std::bad_alloc&) { return kpb_fail(ctx, KPB_E_NOMEM, "%s: out of host memory", what); }
    catch (const KpbwMissing& e) { return kpb_fail(ctx, KPB_E_WEIGHTS, "%s", e.what()); }
    catch (const std::exception& e) { return kpb_fail(ctx, KPB_E_INVALID, "%s: %s", what, e.what()); }
}

struct KpbwRec { char name[40]; uint32_t ndim; uint32_t dims[4]; uint32_t off; };

struct KpbwBlob {
    std::map<std::string, std::pair<const float*, std::vector<uint32_t>>> t;
    uint32_t arch = 0;
    bool parse(const void* blob, size_t len)
    {
        const unsigned char* p = static_cast<const unsigned char*>(blob);
        if (len < 16 || memcmp(p, "KPBWGT1\0", 8) != 0) return false;
        uint32_t n;
        memcpy(&arch, p + 8, 4);
        memcpy(&n, p + 12, 4);
        const size_t base = 16 + (size_t)n * sizeof(KpbwRec);
        if (base > len) return false;
        for (uint32_t i = 0; i < n; ++i) {
            KpbwRec r;
            memcpy(&r, p + 16 + (size_t)i * sizeof(KpbwRec), sizeof(KpbwRec));
            if (r.ndim > 4) return false;
            size_t cnt = 1;
            std::vector<uint32_t> d(r.dims, r.dims + r.ndim);
            for (uint32_t v : d) cnt *= v;
            if (base + 4 * ((size_t)r.off + cnt) > len) return false;
            char nm[41];                      // names may fill all 40 bytes of the field (no terminator then)
            memcpy(nm, r.name, 40);
            nm[40] = 0;
            t[nm] = {reinterpret_cast<const float*>(p + base + 4 * (size_t)r.off), d};
        }
        return true;
    }
    const float* get(const char* name, std::vector<uint32_t> dims) const
    {
        auto it = t.find(name);
        if (it == t.end() || it->second.second != dims) return nullptr;
        return it->second.first;
    }
};

// The one way a create reads a tensor it cannot do without: need() never returns null -- a tensor that is missing or has other dims ends the create with
// KpbwMissing, whose text is the create's refusal sentence `fmt` with the tensor's name for its one %s.  A create binds blob and sentence once, reads in the
// order it wants tensors named, and touches the device only after its last read (WeightStage::upload).  (KpbwBlob::get stays for questions: "is there a ...?")
struct KpbwReader {
    const KpbwBlob& bl;
    const char* fmt;
    const float* need(const std::string& name, std::vector<uint32_t> dims) const
    {
        if (const float* p = bl.get(name.c_str(), std::move(dims))) return p;
        char msg[384];
        snprintf(msg, sizeof(msg), fmt, name.c_str());
        throw KpbwMissing(msg);
    }
};

// host-side staging of repacked tensors, for the nets' creates and kpb_lg_create alike (so its messages name the stage, not a caller).  put() takes a tensor
// together with the pointer member(s) it is to be read through; upload() copies the stage into one device allocation and then assigns every one of them.
// The one rule: a destination is a member of the heap-allocated net or matcher object, which outlives the stage (&net->k2.w1pk, &L.w with L a reference into
// net->L[i]) -- never a member of a local copy, whose address upload() would write through after it is gone.
struct WeightStage {
    struct Bind {
        const float** f = nullptr;
        const uint4** u = nullptr;
        size_t off;
        Bind(const float** d, size_t o) : f(d), off(o) {}
        Bind(const uint4** d, size_t o) : u(d), off(o) {}
    };
    std::vector<float> host;
    std::vector<Bind> binds;    // (destination, offset into host) of every put
    template <class D0, class... D> void put(const std::vector<float>& v, D0 d0, D... d)     // destinations: const float** or const uint4**, at least one
    {
        while (host.size() % 64) host.push_back(0.0f);   // 256-byte alignment for scalar/vector loads
        binds.emplace_back(d0, host.size());
        (binds.emplace_back(d, host.size()), ...);
        host.insert(host.end(), v.begin(), v.end());
    }
    template <class... D> void put_raw(const float* p, size_t n, D... d) { put(std::vector<float>(p, p + n), d...); }
    int upload(kpb_ctx* ctx, float** owner)       // *owner (kpb_net::wdev, kpb_lg::wdev) frees the allocation, also when the upload fails
    {
        if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(owner, host.size() * sizeof(float)) != hipSuccess)
            return kpb_fail(ctx, KPB_E_NOMEM, "WeightStage::upload: weight allocation failed");
        if (hipMemcpy(*owner, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            return kpb_fail(ctx, KPB_E_HIP, "WeightStage::upload: weight copy to the device failed");
        for (const Bind& b : binds) {
            if (b.f) *b.f = *owner + b.off;
            else *b.u = reinterpret_cast<const uint4*>(*owner + b.off);
        }
        return KPB_OK;
    }
};

// (what the conv_mfma networks lend each other -- Layer, stage_layer, launch_mfma, launch_l2norm_nhwc -- is declared in conv_layer.h)

// factories, one per architecture
int alike_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);         // ALIKE-t; hands a blob whose head.w is 129 x 128 to alike_l_create
int alike_l_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);       // ALIKE-l (alike_l.hip)
int superpoint_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int xfeat_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int disk_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int r2d2_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int edgepoint_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int goodpoint_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int letnet_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int keynet_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int sfd2_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int d2net_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
int harris_create(kpb_ctx* ctx, const KpbwBlob& bl, kpb_net** out);
