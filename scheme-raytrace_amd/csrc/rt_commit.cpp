// rt_commit.cpp — rt_scene_commit, the device half: the host scene of rt_build.cpp uploaded, the sizes
// that depend on the device, the LDS kernels' preparation.
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "rt_host.h"
#include "rt_launch.h"
#include "rt_build.h"

using namespace rtamd;

namespace {
#ifdef RT_COMMIT_PROFILE
// what a commit sent to the device, printed after its phases: per array its name, element count and the
// 64-bit FNV-1a hash of its bytes (two builds of the library produce the same device scene or not)
struct Sent { const char* name; const void* p; size_t n, size; };
thread_local std::vector<Sent> tl_sent;
void print_sent() {
    for (const Sent& a : tl_sent) {
        uint64_t x = 1469598103934665603ull;
        for (size_t k = 0; k < a.n * a.size; ++k) x = (x ^ static_cast<const uint8_t*>(a.p)[k]) * 1099511628211ull;
        std::fprintf(stderr, "digest %-10s %10zu %016llx\n", a.name, a.n, (unsigned long long)x);
    }
    tl_sent.clear();
}
#endif

// device time commit_scene spends in upload() (allocation + copy), for rt_scene_info's split of the
// commit into host build and device upload
thread_local double tl_upload_ms = 0.0;
template <class T, class A>
int upload(DevBuf& b, const std::vector<T, A>& v, const T** out, const char* name) {
    const auto t0 = std::chrono::steady_clock::now();
    size_t n = std::max<size_t>(1, v.size()) * sizeof(T);
    HIPCHK(b.ensure(n));
    if (!v.empty()) HIPCHK(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = b.as<const T>();
    tl_upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
#ifdef RT_COMMIT_PROFILE
    tl_sent.push_back({name, v.data(), v.size(), sizeof(T)});
#else
    (void)name;
#endif
    return 0;
}

size_t extend_lds_budget() { return (size_t)64 << 10; }   // largest LDS footprint k_extend_lds may take

// A commit's host scratch (C5: ~0.7 GB of build arrays) takes ~65 ms to unmap on one thread; the commit
// hands it to this worker instead and returns as soon as the device scene is ready.  The worker drains its
// queue before the library unloads.  A forked child inherits the object but not the thread: it starts its
// own and leaves the parent's alone (joining a thread of another process would hang).
class Reaper {
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<std::shared_ptr<void>> q_;
    bool stop_ = false;
    std::thread* th_ = nullptr;
    pid_t pid_ = 0;
    void run() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
            std::vector<std::shared_ptr<void>> batch;
            batch.swap(q_);
            lk.unlock();
            batch.clear();                              // the frees, outside the lock
            lk.lock();
            if (stop_ && q_.empty()) return;
        }
    }
public:
    template <class V>
    void reap(V&& v) {
        auto bundle = std::make_shared<std::decay_t<V>>(std::move(v));
        std::lock_guard<std::mutex> lk(mu_);
        if (!th_ || pid_ != getpid()) {
            th_ = new std::thread([this] { run(); });   // (a parent's thread object stays with the parent)
            pid_ = getpid();
        }
        q_.push_back(std::move(bundle));
        cv_.notify_one();
    }
    ~Reaper() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_one();
        if (th_ && pid_ == getpid()) {
            th_->join();
            delete th_;
        }
    }
};
Reaper g_reaper;

// The curve walk's buffers, sized from the device's CU count: the survivor and hand-off rings, and the
// overflow area of the walk's stack where its deepest stacks spill past the LDS columns
int size_curve_buffers(Scene* s, DevScene& d) {
    // the walk's LDS stack column: kCurveLdsStack entries (a walk rarely holds more; the rest go to the
    // overflow area), so the curve kernel's blocks stay small.  RTAMD_CURVE_LDS_STACK (tests): fewer
    // entries, so the walk exercises its overflow area
    const char* ce = std::getenv("RTAMD_CURVE_LDS_STACK");
    d.lds4 = std::min(d.lane_stack, ce ? std::max(1, std::atoi(ce)) : kCurveLdsStack);
    int dev = 0, cus = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    d.ring_waves = (uint32_t)std::max(cus, 1) * 4u * (uint32_t)kCurveWaves;   // kCurveWaves 256-thread blocks per CU
    HIPCHK(s->d_bez_ring.ensure((size_t)kLanes * d.ring_waves * kBezRing * 128u));
    d.bez_ring = s->d_bez_ring.as<double>();
    HIPCHK(s->d_fuse_ring.ensure((size_t)kLanes * d.ring_waves * kFuseWaveBytes));
    d.fuse_ring = s->d_fuse_ring.as<uint8_t>();
    if (d.stack4 > d.lds4) {
        d.ovf_lanes = (uint32_t)std::max(cus, 1) * 2048u;     // any resident grid of 256-thread blocks
        HIPCHK(s->d_stk_ovf.ensure((size_t)kLanes * d.ovf_lanes * (size_t)(d.stack4 - d.lds4) * sizeof(uint32_t)));
        d.stk_ovf = s->d_stk_ovf.as<uint32_t>();
    }
    return 0;
}

// LDS footprints of the persistent kernels, from the final counts and stack depth in `d` (the kernels
// carve their LDS from the same fields): k_extend_lds, and k_camera (fused raygen + depth-0 extend)
void prepare_lds(Scene* s, const DevScene& d) {
    auto fit = [&](const bool off, const size_t lds, auto prepare, size_t& bytes, uint32_t& blocks) {
        bytes = 0;
        blocks = 0;
        if (off) return;
        uint32_t mb = 0;
        if (lds > 0 && lds <= extend_lds_budget() && prepare(d, lds, &mb) == hipSuccess && mb >= 256) {
            bytes = lds;
            blocks = mb;                  // every resident block (50-88 % of them: -0.3 .. -3 %, profiles/r02/pct)
        }
        (void)hipGetLastError();
    };
    fit(std::getenv("RTAMD_NO_EXTEND_LDS") != nullptr, extend_lds_bytes(d), extend_lds_prepare, s->ext_lds, s->ext_lds_blocks);
    fit(std::getenv("RTAMD_NO_CAMERA_LDS") != nullptr, camera_lds_bytes(d), camera_prepare, s->cam_lds, s->cam_blocks);
}
}  // namespace

namespace rtamd {
int commit_scene(Scene* s, int world) {
#ifdef RT_COMMIT_PROFILE
    commit_t0() = std::chrono::steady_clock::now();
#endif
    CTX_OF(c, s);
    HIPCHK(hipSetDevice(c->device));
    HostScene h;
    std::string err;
    if (build_scene(*s, world, BuildOptions::from_env(), h, err)) return fail(err);
    s->tree = h.tree;
    s->commit_threads = h.threads;
    s->commit_sah_ms = h.sah_ms;
    DevScene& d = s->dev;
    std::memcpy(&d, &h.d, sizeof d);
    int rc = 0;
    auto up = [&](DevBuf& b, const auto& v, auto DevScene::*m, const char* name, const bool present = true) {
        if (present && !rc) rc = upload(b, v, &(d.*m), name);
    };
    const bool tree0 = !h.fbvh2.empty(), gtree0 = !h.g0bvh2.empty() || !h.g0bleaf.empty();
    up(s->d_sph, h.sph, &DevScene::sph, "sph");
    up(s->d_msph, h.msph, &DevScene::msph, "msph");
    up(s->d_rect, h.rect, &DevScene::rect, "rect");
    up(s->d_groups, h.groups, &DevScene::groups, "groups");
    up(s->d_bez, h.bez, &DevScene::bez, "bez");
    up(s->d_klein, h.klein, &DevScene::klein, "klein");
    up(s->d_med, h.med, &DevScene::med, "med");
    up(s->d_bgroups, h.bgroups, &DevScene::bgroups, "bgroups");
    up(s->d_bvh2, h.bvh2, &DevScene::bvh2, "bvh2");
    up(s->d_bleaf, h.bleaf, &DevScene::bleaf, "bleaf");
    up(s->d_fbvh2, h.fbvh2, &DevScene::fbvh2, "fbvh2", tree0);
    up(s->d_fbleaf, h.fbleaf, &DevScene::fbleaf, "fbleaf", tree0);
    up(s->d_fsph, h.fsph, &DevScene::fsph, "fsph", tree0);
    up(s->d_fid, h.fid, &DevScene::fid, "fid", tree0);
    up(s->d_bvh4, h.bvh4, &DevScene::bvh4, "bvh4", !h.bvh4.empty());
    up(s->d_chains, h.chains, &DevScene::chains, "chains");
    up(s->d_leaves, h.leaves, &DevScene::leaves, "leaves");
    up(s->d_leaf_cls, h.leaf_cls, &DevScene::leaf_cls, "leaf_cls");
    up(s->d_order, h.order, &DevScene::order, "order");
    up(s->d_gleaf, h.gleaf, &DevScene::gleaf, "gleaf", h.generic);
    up(s->d_leaf_pos, h.leaf_pos, &DevScene::leaf_pos, "leaf_pos", h.generic);
    up(s->d_rot, h.rot, &DevScene::rot, "rot", h.generic);
    up(s->d_g0bvh2, h.g0bvh2, &DevScene::g0bvh2, "g0bvh2", gtree0);
    up(s->d_g0bleaf, h.g0bleaf, &DevScene::g0bleaf, "g0bleaf", gtree0);
    up(s->d_tri, h.tri, &DevScene::tri, "tri", !h.tri.empty());
    up(s->d_triuv, h.triuv, &DevScene::triuv, "triuv", !h.tri.empty());
    up(s->d_trinrm, h.trinrm, &DevScene::trinrm, "trinrm", h.d.tri_smooth != 0);   // (read behind tri_smooth only)
    up(s->d_lights, h.lights, &DevScene::lights, "lights", !h.lights.empty());
    up(s->d_mats, s->mats, &DevScene::mats, "mats");
    up(s->d_texs, s->texs, &DevScene::texs, "texs");
    up(s->d_teximg, s->teximg, &DevScene::teximg, "teximg", d.has_image_tex != 0);
    up(s->d_ranvec, s->ranvec, &DevScene::ranvec, "ranvec", s->have_perlin);
    up(s->d_perm, s->perm, &DevScene::perm, "perm", s->have_perlin);
    if (rc) return rc;
    if (!h.bvh4.empty())
        if ((rc = size_curve_buffers(s, d))) return rc;
    prepare_lds(s, d);
    // point records hold the point on the world ray: right only where hit_record would take no leaf into an
    // instance chain and the normal needs the point alone (a SOLO world's leaves, checked here all the same)
    s->point_hits = point_hits_scene(d) && (s->ext_lds || s->cam_lds) &&
                    std::all_of(h.leaves.begin(), h.leaves.end(), [](const LeafInfo& li) {
                        return li.chain < 0 && (li.type == LEAF_SPHERE || li.type == LEAF_MSPHERE);
                    });
    HIPCHK(s->d_dev.ensure(sizeof(DevScene)));
    COMMIT_MARK("upload");
    HIPCHK(hipMemcpy(s->d_dev.p, &d, sizeof(DevScene), hipMemcpyHostToDevice));
    s->committed = true;
#ifdef RT_COMMIT_PROFILE
    // DevScene with its pointers null: build_scene's, with what was sized here
    h.d.lds4 = d.lds4; h.d.ring_waves = d.ring_waves; h.d.ovf_lanes = d.ovf_lanes;
    tl_sent.push_back({"DevScene", &h.d, 1, sizeof(DevScene)});
    print_sent();
#endif
    g_reaper.reap(std::move(h));
    return 0;
}
}  // namespace rtamd

extern "C" {

int rt_scene_commit(int scene, int world) {
    SCENE_OR_FAIL(s, scene);
    if (check_obj(s, world)) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    tl_upload_ms = 0.0;
    const int rc = commit_scene(s, world);
#ifdef RT_COMMIT_PROFILE
    std::fprintf(stderr, "commit %-12s %9.1f ms\n", "return",
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
#endif
    s->commit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s->commit_upload_ms = tl_upload_ms;
    return rc;
}

}  // extern "C"
