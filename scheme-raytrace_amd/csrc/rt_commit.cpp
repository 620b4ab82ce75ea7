// rt_commit.cpp — rt_scene_commit: flattening of the reference's object tree into grouped leaves, the
// BVH builds (rt_bvh.h) and the upload of the device scene.
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <tuple>

#include "rt_host.h"
#include "rt_launch.h"
#include "rt_bvh.h"
#include "rt_leafbox.h"

using namespace rtamd;

namespace {
// --------------------------------------------------------- flattening
struct LeafTmp {
    int type;          // LeafType
    int chain;         // -1 = world
    int flip;
    int obj;           // source object
    int aux = -1;      // LEAF_MEDIUM: index into Flattener::bounds
};

struct Flattener {
    Scene* s;
    std::vector<std::vector<ChainOpRec>> chains;   // unique chains
    std::vector<LeafTmp> leaves;                   // DFS order
    std::vector<std::vector<LeafTmp>> bounds;      // per constant medium: its boundary's leaves
    std::vector<ChainOpRec> cur;
    int depth_guard = 0;
    bool in_boundary = false;

    int chain_id() {
        if (cur.empty()) return -1;
        for (size_t i = 0; i < chains.size(); ++i) {
            if (chains[i].size() == cur.size() &&
                std::memcmp(chains[i].data(), cur.data(), cur.size() * sizeof(ChainOpRec)) == 0)
                return (int)i;
        }
        chains.push_back(cur);
        return (int)chains.size() - 1;
    }
    int walk(int id, int flip) {
        if (++depth_guard > 10000) return fail("object graph too deep (cycle?)");
        const Obj& o = s->objs[id];
        int rc = 0;
        switch (o.type) {
        case O_SPHERE: leaves.push_back({LEAF_SPHERE, chain_id(), flip, id}); break;
        case O_MSPHERE: leaves.push_back({LEAF_MSPHERE, chain_id(), flip, id}); break;
        case O_RECT: leaves.push_back({LEAF_RECT_XY + o.axis, chain_id(), flip, id}); break;
        case O_BEZIER:
            if (in_boundary) return fail("a constant medium's boundary may hold spheres, rects, boxes and instances only");
            leaves.push_back({LEAF_BEZIER, chain_id(), flip, id});
            break;
        case O_KLEIN:
            if (in_boundary) return fail("a constant medium's boundary may hold spheres, rects, boxes and instances only");
            leaves.push_back({LEAF_KLEIN, chain_id(), flip, id});
            break;
        case O_MEDIUM: {
            if (in_boundary) return fail("constant media cannot be nested");
            std::vector<LeafTmp> saved;
            saved.swap(leaves);
            in_boundary = true;
            rc = walk(o.child, 0);
            in_boundary = false;
            std::vector<LeafTmp> b;
            b.swap(leaves);
            leaves.swap(saved);
            if (rc) break;
            bounds.push_back(std::move(b));
            LeafTmp L{LEAF_MEDIUM, chain_id(), flip, id};
            L.aux = (int)bounds.size() - 1;
            leaves.push_back(L);
            break;
        }
        case O_FLIP: rc = walk(o.child, flip ^ 1); break;
        case O_BOX:
        case O_LIST:
        case O_BVH:
            for (int k : o.kids) { if ((rc = walk(k, flip))) break; }
            break;
        case O_TRANSLATE:
        case O_ROTATE_Y: {
            if ((int)cur.size() >= kMaxChain) return fail("instance nesting deeper than 4 transforms");
            ChainOpRec op{};
            if (o.type == O_TRANSLATE) { op.op = OP_TRANSLATE; op.x = o.c0[0]; op.y = o.c0[1]; op.z = o.c0[2]; }
            else { op.op = OP_ROTATE_Y; op.x = o.sin_t; op.y = o.cos_t; op.z = 0; }
            cur.push_back(op);
            rc = walk(o.child, flip);
            cur.pop_back();
            break;
        }
        }
        --depth_guard;
        return rc;
    }
};

int bvh_sweep_max(const bool curves) {
    const char* e = std::getenv("RTAMD_BVH_SWEEP");
    return e ? std::atoi(e) : (curves ? 0 : 1 << 16);
}

size_t bvh_min_prims() {
    const char* e = std::getenv("RTAMD_BVH_MIN");
    return e ? (size_t)std::strtoull(e, nullptr, 10) : 16;
}

// fewest generic leaves (rects, instanced spheres) a scene needs for them to join the world tree: below
// the crossover a handful of uniform group loops beats a per-lane walk (the default is
// the measured crossover, 48 leaves, and never below 32; the environment may set any count, for measurements and tests)
constexpr size_t kGenericMinDefault = 48;
static_assert(kGenericMinDefault >= 32, "every scene with fewer generic leaves keeps its groups");
size_t bvh_generic_min() {
    const char* e = std::getenv("RTAMD_BVH_GENERIC_MIN");
    const size_t v = e ? (size_t)std::strtoull(e, nullptr, 10) : kGenericMinDefault;
    return std::min<size_t>(std::max<size_t>(v, 1), (size_t)1 << 30);
}

// device time commit_scene spends in upload() (allocation + copy), for rt_scene_info's split of the
// commit into host build and device upload
thread_local double tl_upload_ms = 0.0;
template <class T, class A>
int upload(DevBuf& b, const std::vector<T, A>& v, const T** out) {
    const auto t0 = std::chrono::steady_clock::now();
    size_t n = std::max<size_t>(1, v.size()) * sizeof(T);
    HIPCHK(b.ensure(n));
    if (!v.empty()) HIPCHK(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = b.as<const T>();
    tl_upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

// An L2 bound on the world-space distance from the origin of every point a
// ray can start from: all leaves (instance chains applied: rotations keep the
// norm, translations add theirs), medium boundaries, the camera; x4 for the
// off-surface points curves report (Q10) and motion extrapolation.
double scene_radius(const Scene* s, const Flattener& f) {
    auto n3 = [](const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    auto chain_len = [&](int ch) {
        double t = 0;
        if (ch >= 0)
            for (const ChainOpRec& op : f.chains[ch])
                if (op.op == OP_TRANSLATE) t += std::sqrt(op.x * op.x + op.y * op.y + op.z * op.z);
        return t;
    };
    auto leaf_r = [&](const LeafTmp& L) {
        const Obj& o = s->objs[L.obj];
        double r = 0;
        switch (L.type) {
        case LEAF_SPHERE: r = n3(o.c0) + std::fabs(o.r); break;
        case LEAF_MSPHERE: r = 2 * std::max(n3(o.c0), n3(o.c1)) + std::fabs(o.r); break;
        case LEAF_BEZIER:
            for (int i = 0; i < 4; ++i) r = std::max(r, n3(o.cp + 3 * i));
            r += std::fabs(o.width);
            break;
        case LEAF_KLEIN: r = n3(o.c0) + 1200; break;
        case LEAF_MEDIUM: r = 0; break;
        default:
            r = std::sqrt(3.0) * std::max({std::fabs(o.a0), std::fabs(o.a1), std::fabs(o.b0), std::fabs(o.b1),
                                           std::fabs(o.k)});
        }
        return r + chain_len(L.chain);
    };
    double R = n3(s->cam + 9) + std::fabs(s->cam[21]);
    const int nt = build_threads();
    std::vector<double> part((size_t)nt, R);        // (max is order-free: a NaN radius never enters)
    parallel_for(f.leaves.size(), nt, [&](const size_t b, const size_t e) {
        double r = R;
        for (size_t i = b; i < e; ++i) r = std::max(r, leaf_r(f.leaves[i]));
        part[b / std::max<size_t>(1, (f.leaves.size() + (size_t)nt - 1) / (size_t)nt)] = r;
    });
    for (const double r : part) R = std::max(R, r);
    for (const auto& b : f.bounds) for (const LeafTmp& L : b) R = std::max(R, leaf_r(L));
    return 4 * R + 1;
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
    template <class... V>
    void reap(V&&... v) {
        auto bundle = std::make_shared<std::tuple<std::decay_t<V>...>>(std::move(v)...);
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
}  // namespace

namespace rtamd {
#ifdef RT_COMMIT_PROFILE
#define COMMIT_MARK(tag) std::fprintf(stderr, "commit %-12s %9.1f ms\n", tag, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - cp0).count())
#else
#define COMMIT_MARK(tag) ((void)0)
#endif
int commit_scene(Scene* s, int world) {
#ifdef RT_COMMIT_PROFILE
    const auto cp0 = std::chrono::steady_clock::now();
#endif
    CTX_OF(c, s);
    HIPCHK(hipSetDevice(c->device));
    if (!s->have_cam) return fail("rt_scene_commit: no camera set (rt_set_camera)");
    for (const auto& t : s->texs)
        if ((t.type == TEX_NOISE || t.type == TEX_MARBLE) && !s->have_perlin)
            return fail("rt_scene_commit: noise/marble texture needs rt_set_perlin_tables");
    Flattener f{s};
    f.leaves.reserve(s->objs.size());                // (a hint: an object listed twice is two leaves)
    if (int rc = f.walk(world, 0)) return rc;

    // group leaves by (chain, type) in first-appearance order of chains
    std::vector<int> chain_order;   // -1 first
    chain_order.push_back(-1);
    for (size_t i = 0; i < f.chains.size(); ++i) chain_order.push_back((int)i);
    HostVec<SphereRec> sph;                          // (filled by threads after a resize: rt_bvh.h, NoInit)
    HostVec<MSphereRec> msph;
    std::vector<RectRec> rect;
    std::vector<Group> groups;
    HostVec<LeafInfo> lsph, lmsph;
    std::vector<LeafInfo> lrect[3];

    HostVec<BezierRec> bez;
    HostVec<LeafInfo> lbez;
    std::vector<KleinRec> klein;
    std::vector<LeafInfo> lklein;
    auto bezier_rec = [](const Obj& o) {
        BezierRec b{};
        for (int k = 0; k < 12; ++k) b.cp[k] = o.cp[k];
        b.w1 = o.width / 2;                 // bezier.scm:63-65
        b.w2 = b.w1 * b.w1;
        b.eps8 = 8 * (o.width / 20);
        return b;
    };

    // A constant medium draws a random number inside its hit test, so its
    // position in the object list matters (the draw happens only if the
    // closest hit so far leaves part of its span): the leaves are cut into
    // segments at each medium and evaluated segment by segment, each medium
    // right after the objects that precede it.  Within a segment the order of
    // the other primitives does not change the closest hit.
    std::vector<int> seg(f.leaves.size(), 0);
    int nseg = 1;
    for (size_t i = 0; i < f.leaves.size(); ++i) {
        seg[i] = nseg - 1;
        if (f.leaves[i].type == LEAF_MEDIUM) ++nseg;
    }

    // BVH over the world-level (chain -1) spheres, moving spheres and curves of segment 0
    COMMIT_MARK("flatten");
    const int threads = build_threads();
    std::vector<int> in_bvh;                         // the leaves the BVH takes, in list order
    size_t n_world = 0;                              // of them, world-level spheres / moving spheres / curves
    for (size_t i = 0; i < f.leaves.size(); ++i) {
        const LeafTmp& L = f.leaves[i];
        if (seg[i] == 0 && L.chain == -1 && (L.type == LEAF_SPHERE || L.type == LEAF_MSPHERE || L.type == LEAF_BEZIER))
            in_bvh.push_back((int)i);
    }
    n_world = in_bvh.size();
    // Generic tree leaves (include/rt.h, rt_add_bvh): rects under any chain or none and spheres / moving
    // spheres under a chain, with a finite world-space box (rt_leafbox.h), in scenes of spheres, moving
    // spheres and rects only.  A rect also needs its chain's rotation in the table the kernels test a
    // ray's direction against (RotEntry; at most kMaxRot).  They join the tree when there are at least
    // bvh_generic_min() of them and the tree is built at all; else nothing below differs from a commit
    // without them.
    const double cam_tlo = std::min(std::min(s->cam[22], s->cam[23]), 0.0);
    const double cam_thi = std::max(std::max(s->cam[22], s->cam[23]), 0.0);
    auto leaf_geom = [&](const LeafTmp& L) {
        const Obj& o = s->objs[L.obj];
        LeafGeom g{};
        g.type = L.type;
        for (int k = 0; k < 3; ++k) { g.c0[k] = o.c0[k]; g.c1[k] = o.c1[k]; }
        g.r = o.r; g.t0 = o.t0; g.t1 = o.t1;
        g.a0 = o.a0; g.a1 = o.a1; g.b0 = o.b0; g.b1 = o.b1; g.k = o.k;
        return g;
    };
    auto chain_ops = [&](const int ch, int& n) -> const ChainOpRec* {
        n = ch >= 0 ? (int)f.chains[ch].size() : 0;
        return ch >= 0 ? f.chains[ch].data() : nullptr;
    };
    const size_t gen_min = bvh_generic_min();
    std::vector<RotEntry> rot;
    std::vector<PrimRef> gen_ref;                    // a generic leaf's box, by list position
    std::vector<char> is_gen;
    size_t n_gen = 0;
    bool plain = nseg == 1 && f.bounds.empty();
    for (const LeafTmp& L : f.leaves) plain = plain && L.type != LEAF_BEZIER && L.type != LEAF_KLEIN && L.type != LEAF_MEDIUM;
    if (plain && f.leaves.size() >= gen_min) {
        gen_ref.resize(f.leaves.size());
        is_gen.assign(f.leaves.size(), 0);
        for (size_t i = 0; i < f.leaves.size(); ++i) {
            const LeafTmp& L = f.leaves[i];
            const bool is_rect = L.type >= LEAF_RECT_XY && L.type <= LEAF_RECT_YZ;
            if (!is_rect && L.chain < 0) continue;
            int n_ops = 0;
            const ChainOpRec* ops = chain_ops(L.chain, n_ops);
            PrimRef r{};
            if (!leaf_world_box(leaf_geom(L), ops, n_ops, cam_tlo, cam_thi, r.lo, r.hi)) continue;
            if (is_rect) {
                RotEntry e{};
                for (int k = 0; k < n_ops; ++k)
                    if (ops[k].op == OP_ROTATE_Y) { e.sc[e.n][0] = ops[k].x; e.sc[e.n][1] = ops[k].y; ++e.n; }
                size_t at = 0;
                while (at < rot.size() && (rot[at].n != e.n || std::memcmp(rot[at].sc, e.sc, sizeof e.sc) != 0)) ++at;
                if (at == rot.size()) {
                    if (rot.size() >= (size_t)kMaxRot) continue;       // the table is full: the rect keeps its group
                    rot.push_back(e);
                }
                rot[at].axes |= L.type == LEAF_RECT_YZ ? 1 : L.type == LEAF_RECT_XZ ? 2 : 4;   // the plane's normal
            }
            for (int k = 0; k < 3; ++k) r.c[k] = 0.5 * (r.lo[k] + r.hi[k]);
            r.leaf = (int)i;
            r.type = L.type;
            gen_ref[i] = r;
            is_gen[i] = 1;
            ++n_gen;
        }
    }
    const bool generic = n_gen > 0 && n_gen >= gen_min && n_world + n_gen >= bvh_min_prims();
    if (generic) {
        in_bvh.clear();
        for (size_t i = 0; i < f.leaves.size(); ++i) {
            const LeafTmp& L = f.leaves[i];
            if (is_gen[i] || (L.chain == -1 && (L.type == LEAF_SPHERE || L.type == LEAF_MSPHERE))) in_bvh.push_back((int)i);
        }
    }
    std::vector<PrimRef> refs(in_bvh.size());
    parallel_for(in_bvh.size(), threads, [&](const size_t jb, const size_t je) {
      for (size_t j = jb; j < je; ++j) {
        const size_t i = (size_t)in_bvh[j];
        const LeafTmp& L = f.leaves[i];
        const Obj& o = s->objs[L.obj];
        if (generic && is_gen[i]) { refs[j] = gen_ref[i]; continue; }
        PrimRef r{};
        r.leaf = (int)i;
        r.type = L.type;
        const double rad = std::fabs(o.r);
        if (L.type == LEAF_SPHERE) {
            for (int k = 0; k < 3; ++k) { r.lo[k] = o.c0[k] - rad; r.hi[k] = o.c0[k] + rad; }
        } else if (L.type == LEAF_BEZIER) {
            const double w1 = std::fabs(o.width / 2);
            for (int k = 0; k < 3; ++k) {
                r.lo[k] = std::min(std::min(o.cp[k], o.cp[3 + k]), std::min(o.cp[6 + k], o.cp[9 + k])) - w1;
                r.hi[k] = std::max(std::max(o.cp[k], o.cp[3 + k]), std::max(o.cp[6 + k], o.cp[9 + k])) + w1;
            }
        } else {
            const double den = o.t1 - o.t0;
            const double ct0 = s->cam[22], ct1 = s->cam[23];
            const double tlo = std::min(std::min(ct0, ct1), 0.0), thi = std::max(std::max(ct0, ct1), 0.0);
            if (!(den != 0.0) || !std::isfinite(den)) {
                for (int k = 0; k < 3; ++k) { r.lo[k] = -1e300; r.hi[k] = 1e300; }
            } else {
                const double f0 = (tlo - o.t0) / den, f1 = (thi - o.t0) / den;
                for (int k = 0; k < 3; ++k) {
                    const double dc = o.c1[k] - o.c0[k];
                    const double a = o.c0[k] + dc * f0, b = o.c0[k] + dc * f1;
                    r.lo[k] = std::min(a, b) - rad; r.hi[k] = std::max(a, b) + rad;
                }
            }
        }
        pad_box(r.lo, r.hi);
        for (int k = 0; k < 3; ++k) r.c[k] = 0.5 * (r.lo[k] + r.hi[k]);
        refs[j] = r;
      }
    });
    COMMIT_MARK("refs");
    // list position -> (type, index in the type's array) of every world leaf (DevScene::order)
    std::vector<int32_t> ord_type(f.leaves.size(), -1), ord_local(f.leaves.size(), -1);
    const bool use_bvh = !refs.empty() && refs.size() >= bvh_min_prims();
    std::vector<BvhNode> bvh_nodes;
    HostVec<BvhNode2> bvh2;
    HostVec<BvhLeaf> bleaf;
    int32_t bvh2_root = 0;
    int32_t lane_stack = 0;
    HostVec<BvhNode4> bvh4;                          // curve trees (k_extend_curves)
    int32_t bvh4_root = 0, stack4 = 0;
    bool bvh_has_bez = false;
    float bvh_pad = 0.0f;
    double margin = 0.0;
    HostVec<BvhNode2> fbvh2;                         // time-0 tree (see below)
    HostVec<BvhLeaf> fbleaf;
    std::vector<SphereRec> fsph;
    std::vector<std::pair<int, int>> fsrc;           // (LEAF_SPHERE | LEAF_MSPHERE, local)
    int32_t fbvh2_root = 0;
    bool tree0_any_time = false;
    bool tree0_direct = false;
    // generic tree leaves: (type, local) of ref i, then of the time-0 tree's ref i (-> DevScene::gleaf);
    // the time-0 tree itself
    std::vector<std::pair<int, int>> gsrc;
    HostVec<BvhNode2> g0bvh2;
    HostVec<BvhLeaf> g0bleaf;
    int32_t g0bvh2_root = 0, depth_all = 0, depth0 = 0;
    if (use_bvh) {
        BvhBuild bb{refs, {}};
        // one primitive per leaf (measured fastest for sphere trees; for C5's curve tree, with the exact
        // SAH sweep below 65 536 primitives, +1.5 % / +0.6 % over two per leaf: profiles/r02/ab_c5,
        // profiles/r03/c5walk/ab_leaf1.log)
        bb.leaf_max = 1;
        bb.sweep_max = bvh_sweep_max(bb.leaf_max > 1 &&
                                     std::any_of(refs.begin(), refs.end(), [](const PrimRef& r) { return r.type == LEAF_BEZIER; }));
        bb.threads = threads;
        s->commit_threads = bb.threads;
        const auto ts = std::chrono::steady_clock::now();
        bb.build(0, (int)refs.size(), 0);
        s->commit_sah_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts).count();
        COMMIT_MARK("sah");
        // leaf ranges: refs order -> sphere / moving-sphere / curve array indices
        std::vector<int> ns(refs.size() + 1, 0), nm(refs.size() + 1, 0), nb(refs.size() + 1, 0);
        for (size_t i = 0; i < refs.size(); ++i) {
            ns[i + 1] = ns[i] + (refs[i].type == LEAF_SPHERE);
            nm[i + 1] = nm[i] + (refs[i].type == LEAF_MSPHERE);
            nb[i + 1] = nb[i] + (refs[i].type == LEAF_BEZIER);
        }
        bvh_has_bez = nb[refs.size()] > 0;
        bvh_nodes = std::move(bb.nodes);
        COMMIT_MARK("prefix");
        // f32 box margin: 2^-21 x a radius bound R on everything a ray can start
        // from (x4 included, see scene_radius).  The slab ends carry at most
        // ~4 ulps x (|box| + |o|) <= 2^-22 x 1.25 R of rounding; the margin is
        // 1.6x that.
        margin = std::ldexp(scene_radius(s, f), -21);
        bvh_pad = (float)margin;
        COMMIT_MARK("radius");
        flatten_bvh2(bvh_nodes, margin, [&](int b, int e) {
            if (generic) return BvhLeaf{0, 0, 0, 0, 0, 0, b, e - b};      // every leaf by its id (gleaf)
            return BvhLeaf{ns[b], ns[e] - ns[b], nm[b], nm[e] - nm[b], nb[b], nb[e] - nb[b], 0, 0};
        }, bvh2, bleaf, bvh2_root, lane_stack, threads);
        depth_all = lane_stack;
        COMMIT_MARK("flatten2");
        if (bvh_has_bez) {                               // single-curve leaves: direct refs (kDirectCurve)
            auto direct = [&](int32_t& ref) {
                if (ref >= 0) return;
                const BvhLeaf& L = bleaf[~ref];
                if (L.sn == 0 && L.mn == 0 && L.bn == 1 && L.bb < kDirectCurve) ref = ~(kDirectCurve + L.bb);
            };
            for (BvhNode2& M : bvh2) { direct(M.l); direct(M.r); }
            direct(bvh2_root);
            COMMIT_MARK("bvh2");
            bvh4_root = collapse_bvh4(bvh2, bvh2_root, bvh4, stack4, threads);
            COMMIT_MARK("bvh4");
        }
        groups.push_back(Group{GROUP_BVH, -1, 0, (int)bvh_nodes.size()});
        // records in refs order: ref i is sphere ns[i] / moving sphere nm[i] / curve nb[i] of its type's
        // arrays (the prefix counts above), so the refs fill them independently, on the build's threads
        sph.resize((size_t)ns[refs.size()]); lsph.resize(sph.size());
        msph.resize((size_t)nm[refs.size()]); lmsph.resize(msph.size());
        bez.resize((size_t)nb[refs.size()]); lbez.resize(bez.size());
        COMMIT_MARK("resize");
        parallel_for(refs.size(), bb.threads, [&](const size_t b, const size_t e) {
            for (size_t i = b; i < e; ++i) {
                const PrimRef& r = refs[i];
                const LeafTmp& L = f.leaves[r.leaf];
                const Obj& o = s->objs[L.obj];
                LeafInfo li{};
                li.type = L.type; li.chain = L.chain; li.mat = o.mat; li.flip = L.flip;
                if (r.type >= LEAF_RECT_XY && r.type <= LEAF_RECT_YZ) continue;      // (generic: below)
                if (r.type == LEAF_SPHERE) {
                    li.inv_r = 1.0 / o.r;
                    li.local = ns[i];
                    sph[(size_t)ns[i]] = SphereRec{o.c0[0], o.c0[1], o.c0[2], o.r * o.r};
                    lsph[(size_t)ns[i]] = li;
                } else if (r.type == LEAF_MSPHERE) {
                    li.inv_r = 1.0 / o.r;
                    li.local = nm[i];
                    MSphereRec m{};
                    m.c0x = o.c0[0]; m.c0y = o.c0[1]; m.c0z = o.c0[2]; m.rr = o.r * o.r;
                    m.dcx = o.c1[0] - o.c0[0]; m.dcy = o.c1[1] - o.c0[1]; m.dcz = o.c1[2] - o.c0[2];
                    m.t0 = o.t0; m.den = o.t1 - o.t0;
                    msph[(size_t)nm[i]] = m;
                    lmsph[(size_t)nm[i]] = li;
                } else {
                    li.local = nb[i];
                    bez[(size_t)nb[i]] = bezier_rec(o);
                    bez[(size_t)nb[i]].order = (uint32_t)r.leaf;      // the flattened list position
                    lbez[(size_t)nb[i]] = li;
                }
                ord_type[(size_t)r.leaf] = r.type;
                ord_local[(size_t)r.leaf] = li.local;
            }
        });
        if (generic) {
            gsrc.resize(refs.size());
            for (size_t i = 0; i < refs.size(); ++i) {
                const PrimRef& r = refs[i];
                if (r.type == LEAF_SPHERE) { gsrc[i] = {LEAF_SPHERE, ns[i]}; continue; }
                if (r.type == LEAF_MSPHERE) { gsrc[i] = {LEAF_MSPHERE, nm[i]}; continue; }
                const LeafTmp& L = f.leaves[r.leaf];                          // a rect: records in refs order
                const Obj& o = s->objs[L.obj];
                LeafInfo li{};
                li.type = L.type; li.chain = L.chain; li.mat = o.mat; li.flip = L.flip;
                li.local = (int)rect.size();
                RectRec R{};
                R.a0 = o.a0; R.a1 = o.a1; R.b0 = o.b0; R.b1 = o.b1; R.k = o.k;
                rect.push_back(R);
                lrect[L.type - LEAF_RECT_XY].push_back(li);
                ord_type[(size_t)r.leaf] = L.type;
                ord_local[(size_t)r.leaf] = li.local;
                gsrc[i] = {L.type, li.local};
            }
            // The time-0 tree of a scene with generic leaves: the same leaves, every moving sphere (under a
            // chain or not) bounded where it is at time 0; none when no sphere moves.  A moving sphere's
            // test at time +0.0 is the all-times one, so only the boxes differ.
            if (nm[refs.size()] > 0 && !std::getenv("RTAMD_NO_BVH0")) {
                std::vector<PrimRef> refs0(refs);
                for (size_t i = 0; i < refs0.size(); ++i) {
                    PrimRef& r = refs0[i];
                    const LeafTmp& L = f.leaves[r.leaf];
                    r.leaf = (int)i;                                          // index into refs (-> gsrc)
                    if (r.type != LEAF_MSPHERE) continue;
                    int n_ops = 0;
                    const ChainOpRec* ops = chain_ops(L.chain, n_ops);
                    double lo[3], hi[3];
                    if (!leaf_world_box(leaf_geom(L), ops, n_ops, 0.0, 0.0, lo, hi)) continue;   // keeps the all-times box
                    for (int k = 0; k < 3; ++k) { r.lo[k] = lo[k]; r.hi[k] = hi[k]; r.c[k] = 0.5 * (lo[k] + hi[k]); }
                }
                BvhBuild b0{refs0, {}};
                b0.leaf_max = bb.leaf_max;
                b0.trav_cost = bb.trav_cost;
                b0.sweep_max = bb.sweep_max;
                b0.threads = bb.threads;
                const auto t0s = std::chrono::steady_clock::now();
                b0.build(0, (int)refs0.size(), 0);
                s->commit_sah_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0s).count();
                const int nr = (int)refs.size();
                flatten_bvh2(b0.nodes, margin, [&](int b, int e) { return BvhLeaf{0, 0, 0, 0, 0, 0, nr + b, e - b}; },
                             g0bvh2, g0bleaf, g0bvh2_root, depth0);
                lane_stack = std::max(lane_stack, depth0);
                for (const PrimRef& r : refs0) gsrc.push_back(gsrc[(size_t)r.leaf]);
            }
        }
        // Time-0 BVH.  Every scattered ray has time 0 (make-ray, ray.scm:8-9,
        // Q4), so for those rays a moving sphere sits at center(0) exactly:
        // the second tree bounds each moving sphere at that one position
        // instead of over the whole shutter, and stores it as a plain sphere
        // whose center is computed here with the kernel's own operations
        // (c0 + dc * ((0 - t0) / den), IEEE f64, no contraction), so the
        // primitive test it runs is bit-for-bit the moving-sphere test.
        // (Built for every sphere tree: with no moving spheres it equals the
        // all-times tree and serves every ray, tree0_any_time.)
        tree0_any_time = nm[refs.size()] == 0;
        if (!bvh_has_bez && !generic && !std::getenv("RTAMD_NO_BVH0")) {
            std::vector<PrimRef> refs0;
            for (size_t i = 0; i < refs.size(); ++i) {
                PrimRef r = refs[i];
                r.leaf = (int)i;                     // index into refs (-> fsph / fid below)
                if (r.type == LEAF_MSPHERE) {
                    const MSphereRec& m = msph[(size_t)nm[i]];
                    const double frac = (0.0 - m.t0) / m.den;
                    const double c[3] = {m.c0x + m.dcx * frac, m.c0y + m.dcy * frac, m.c0z + m.dcz * frac};
                    const double rad = std::sqrt(m.rr) * (1 + 1e-15) + 1e-300;
                    const bool fin = std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]);
                    for (int k = 0; k < 3; ++k) {
                        r.lo[k] = fin ? c[k] - rad : -1e300;
                        r.hi[k] = fin ? c[k] + rad : 1e300;
                    }
                    pad_box(r.lo, r.hi);
                    for (int k = 0; k < 3; ++k) r.c[k] = 0.5 * (r.lo[k] + r.hi[k]);
                }
                refs0.push_back(r);
            }
            BvhBuild b0{refs0, {}};
            b0.leaf_max = bb.leaf_max;
            b0.trav_cost = bb.trav_cost;
            b0.sweep_max = bb.sweep_max;
            b0.singles = b0.leaf_max == 1;           // direct leaves (below) need one sphere per leaf
            b0.threads = bb.threads;
            const auto t0s = std::chrono::steady_clock::now();
            b0.build(0, (int)refs0.size(), 0);
            s->commit_sah_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0s).count();
            // fsph in refs0 order; each entry remembers which sphere / moving sphere it is
            for (const PrimRef& r : refs0) {
                const size_t i = (size_t)r.leaf;
                if (r.type == LEAF_SPHERE) {
                    fsph.push_back(sph[(size_t)ns[i]]);
                    fsrc.push_back({LEAF_SPHERE, ns[i]});
                } else {
                    const MSphereRec& m = msph[(size_t)nm[i]];
                    const double frac = (0.0 - m.t0) / m.den;
                    fsph.push_back({m.c0x + m.dcx * frac, m.c0y + m.dcy * frac, m.c0z + m.dcz * frac, m.rr});
                    fsrc.push_back({LEAF_MSPHERE, nm[i]});
                }
            }
            flatten_bvh2(b0.nodes, margin, [&](int b, int e) { return BvhLeaf{b, e - b, 0, 0, 0, 0, 0, 0}; },
                         fbvh2, fbleaf, fbvh2_root, depth0);
            lane_stack = std::max(lane_stack, depth0);
            // Direct leaves: when every time-0 leaf holds exactly one sphere, put
            // fsph (and its leaf-id map) in leaf order, so leaf k is sphere k and
            // the SOLO LDS kernels need no leaf records (DevScene::bvh_solo).
            tree0_direct = std::all_of(fbleaf.begin(), fbleaf.end(), [](const BvhLeaf& L) { return L.sn == 1; });
            if (tree0_direct) {
                std::vector<SphereRec> fs2(fbleaf.size());
                std::vector<std::pair<int, int>> src2(fbleaf.size());
                for (size_t k = 0; k < fbleaf.size(); ++k) {
                    fs2[k] = fsph[(size_t)fbleaf[k].sb];
                    src2[k] = fsrc[(size_t)fbleaf[k].sb];
                    fbleaf[k].sb = (int32_t)k;
                }
                fsph.swap(fs2);
                fsrc.swap(src2);
            }
        }
    }
    COMMIT_MARK("records");
    std::vector<MediumRec> med;
    std::vector<LeafInfo> lmed;
    std::vector<Group> bgroups;
    // records of one leaf.  Leaf id = leaf_base[type] + index in the type's
    // record array, so every record gets a LeafInfo; boundary leaves (never a
    // closest hit) get a placeholder.
    auto add_record = [&](const LeafTmp& L, LeafInfo* li_world) {
        const Obj& o = s->objs[L.obj];
        LeafInfo placeholder{};
        placeholder.type = L.type; placeholder.chain = -1; placeholder.mat = 0;
        LeafInfo* li = li_world ? li_world : &placeholder;
        if (L.type == LEAF_SPHERE) {
            li->local = (int)sph.size(); li->inv_r = 1.0 / o.r;  lsph.push_back(*li);
            sph.push_back({o.c0[0], o.c0[1], o.c0[2], o.r * o.r});
        } else if (L.type == LEAF_MSPHERE) {
            MSphereRec m{};
            m.c0x = o.c0[0]; m.c0y = o.c0[1]; m.c0z = o.c0[2]; m.rr = o.r * o.r;
            m.dcx = o.c1[0] - o.c0[0]; m.dcy = o.c1[1] - o.c0[1]; m.dcz = o.c1[2] - o.c0[2];
            m.t0 = o.t0; m.den = o.t1 - o.t0;
            li->local = (int)msph.size(); li->inv_r = 1.0 / o.r;  lmsph.push_back(*li);
            msph.push_back(m);
        } else if (L.type == LEAF_BEZIER) {
            li->local = (int)bez.size(); lbez.push_back(*li);
            bez.push_back(bezier_rec(o));
            {   // the flattened list position (medium boundaries come from f.bounds: order 0, ties irrelevant)
                const uintptr_t p = reinterpret_cast<uintptr_t>(&L), b0 = reinterpret_cast<uintptr_t>(f.leaves.data());
                const bool in_list = p >= b0 && p < b0 + f.leaves.size() * sizeof(LeafTmp);
                bez.back().order = in_list ? (uint32_t)((p - b0) / sizeof(LeafTmp)) : 0u;
            }
        } else if (L.type == LEAF_KLEIN) {
            li->local = (int)klein.size(); lklein.push_back(*li);
            klein.push_back({o.c0[0], o.c0[1], o.c0[2], 0.0});
        } else {
            RectRec r{};
            r.a0 = o.a0; r.a1 = o.a1; r.b0 = o.b0; r.b1 = o.b1; r.k = o.k;
            li->local = (int)rect.size(); lrect[L.type - LEAF_RECT_XY].push_back(*li);
            rect.push_back(r);
        }
        if (li_world) {                                 // a world leaf: L is an element of f.leaves
            const size_t at = (size_t)(&L - f.leaves.data());
            ord_type[at] = L.type;
            ord_local[at] = li->local;
        }
    };
    auto type_size = [&](int type) {
        return (type == LEAF_SPHERE) ? sph.size() : (type == LEAF_MSPHERE) ? msph.size()
             : (type == LEAF_BEZIER) ? bez.size() : (type == LEAF_KLEIN) ? klein.size() : rect.size();
    };
    // group a leaf subset by (chain, type) into `out`; world leaves also get LeafInfo
    auto emit_groups = [&](const std::vector<const LeafTmp*>& ls, std::vector<Group>& out, bool world, bool skip_bvh) {
        for (int ch : chain_order) {
            for (int type = LEAF_SPHERE; type <= LEAF_KLEIN; ++type) {
                if (type == LEAF_MEDIUM) continue;
                if (skip_bvh && ch == -1 && (type == LEAF_SPHERE || type == LEAF_MSPHERE || type == LEAF_BEZIER)) continue;
                Group g{type, ch, 0, 0};
                const size_t before = type_size(type);
                g.begin = (int)before;
                for (const LeafTmp* L : ls) {
                    if (L->chain != ch || L->type != type) continue;
                    if (world && generic && is_gen[(size_t)(L - f.leaves.data())]) continue;   // in the tree
                    if (world) {
                        LeafInfo li{};
                        li.type = type; li.chain = ch; li.mat = s->objs[L->obj].mat; li.flip = L->flip;
                        add_record(*L, &li);
                    } else {
                        add_record(*L, nullptr);
                    }
                }
                const size_t after = type_size(type);
                g.end = (int)after;
                if (after > before) out.push_back(g);
            }
        }
    };
    for (int sg = 0; sg < nseg; ++sg) {
        std::vector<const LeafTmp*> ls;
        const LeafTmp* medium = nullptr;
        for (size_t i = 0; i < f.leaves.size(); ++i) {
            if (seg[i] != sg) continue;
            if (f.leaves[i].type == LEAF_MEDIUM) medium = &f.leaves[i];
            else ls.push_back(&f.leaves[i]);
        }
        emit_groups(ls, groups, true, use_bvh && sg == 0);
        COMMIT_MARK("emit");
        if (!medium) continue;
        const Obj& o = s->objs[medium->obj];
        MediumRec m{};
        m.bg_begin = (int)bgroups.size();
        std::vector<const LeafTmp*> bl;
        for (const LeafTmp& L : f.bounds[medium->aux]) bl.push_back(&L);
        emit_groups(bl, bgroups, false, false);
        m.bg_end = (int)bgroups.size();
        m.neg_inv_density = -(1 / o.r);             // (- (/ 1 density)), geometry.scm:564
        LeafInfo li{};
        li.type = LEAF_MEDIUM; li.chain = medium->chain; li.local = (int)med.size();
        li.mat = o.mat; li.flip = medium->flip;
        groups.push_back(Group{LEAF_MEDIUM, medium->chain, (int)med.size(), (int)med.size() + 1});
        med.push_back(m);
        lmed.push_back(li);
    }
    if (lsph.size() != sph.size() || lmsph.size() != msph.size() || lbez.size() != bez.size() ||
        lklein.size() != klein.size() ||
        lrect[0].size() + lrect[1].size() + lrect[2].size() != rect.size())
        return fail("internal: leaf records and leaf infos out of step");
    // leaf ids: spheres, moving spheres, then all rects (rect locals index the shared rect array)
    // rect arrays are shared between the three axis types; leaf id = rect_base + local
    std::vector<LeafInfo> rl(rect.size());
    for (int a = 0; a < 3; ++a) for (auto& li : lrect[a]) rl[li.local] = li;
    int32_t base[kLeafTypes];
    base[LEAF_SPHERE] = 0;
    base[LEAF_MSPHERE] = base[LEAF_SPHERE] + (int32_t)lsph.size();
    base[LEAF_RECT_XY] = base[LEAF_RECT_XZ] = base[LEAF_RECT_YZ] = base[LEAF_MSPHERE] + (int32_t)lmsph.size();
    base[LEAF_BEZIER] = base[LEAF_RECT_XY] + (int32_t)rl.size();
    base[LEAF_MEDIUM] = base[LEAF_BEZIER] + (int32_t)lbez.size();
    base[LEAF_KLEIN] = base[LEAF_MEDIUM] + (int32_t)lmed.size();
    HostVec<LeafInfo> leaves;
    leaves.resize((size_t)base[LEAF_KLEIN] + lklein.size());
    auto put = [&](const LeafInfo* src, const size_t n, const int32_t at) {
        parallel_for(n, threads, [&](const size_t b, const size_t e) { std::copy(src + b, src + e, leaves.data() + at + b); });
    };
    put(lsph.data(), lsph.size(), base[LEAF_SPHERE]);
    put(lmsph.data(), lmsph.size(), base[LEAF_MSPHERE]);
    put(rl.data(), rl.size(), base[LEAF_RECT_XY]);
    put(lbez.data(), lbez.size(), base[LEAF_BEZIER]);
    put(lmed.data(), lmed.size(), base[LEAF_MEDIUM]);
    put(lklein.data(), lklein.size(), base[LEAF_KLEIN]);
    COMMIT_MARK("leaves");
    // the shade-side fields: material, texture shortcut, sphere centre (LeafInfo)
    parallel_for(leaves.size(), threads, [&](const size_t lb, const size_t le) {
      for (size_t lk = lb; lk < le; ++lk) {
        LeafInfo& li = leaves[lk];
        if (li.mat < 0 || li.mat >= (int)s->mats.size()) continue;     // boundary placeholders
        const DevMaterial& m = s->mats[li.mat];
        li.mtype = m.type;
        li.tex = m.tex;
        li.mparam = (m.type == MAT_METAL) ? m.fuzz : m.ref_idx;
        li.tex_kind = TK_GENERIC;
        auto constant = [&](int t) { return t >= 0 && t < (int)s->texs.size() && s->texs[t].type == TEX_CONSTANT; };
        if (constant(m.tex)) {
            const DevTexture& T = s->texs[m.tex];
            li.tex_kind = TK_CONSTANT;
            li.albedo[0] = T.r; li.albedo[1] = T.g; li.albedo[2] = T.bl;
        } else if (m.tex >= 0 && m.tex < (int)s->texs.size() && s->texs[m.tex].type == TEX_CHECKER &&
                   constant(s->texs[m.tex].a) && constant(s->texs[m.tex].b)) {
            const DevTexture& E = s->texs[s->texs[m.tex].a];       // even (texture.scm:20-23)
            const DevTexture& O = s->texs[s->texs[m.tex].b];       // odd
            li.tex_kind = TK_CHECKER_CONST;
            li.albedo[0] = E.r; li.albedo[1] = E.g; li.albedo[2] = E.bl;
            li.albedo2[0] = O.r; li.albedo2[1] = O.g; li.albedo2[2] = O.bl;
        }
        if (li.type == LEAF_SPHERE) {
            const SphereRec& S = sph[(size_t)li.local];
            li.c[0] = S.cx; li.c[1] = S.cy; li.c[2] = S.cz;
        } else if (li.type == LEAF_MSPHERE) {                   // center(0), the kernel's own operations
            const MSphereRec& M = msph[(size_t)li.local];
            const double frac = (0.0 - M.t0) / M.den;
            li.c[0] = M.c0x + M.dcx * frac; li.c[1] = M.c0y + M.dcy * frac; li.c[2] = M.c0z + M.dcz * frac;
        }
      }
    });

    std::vector<Chain> chains;
    for (auto& cv : f.chains) {
        Chain c{};
        c.n = (int)cv.size();
        for (size_t k = 0; k < cv.size(); ++k) c.ops[k] = cv[k];
        chains.push_back(c);
    }
    DevScene& d = s->dev;
    std::memset(&d, 0, sizeof d);
    COMMIT_MARK("groups");
    if (int rc = upload(s->d_sph, sph, &d.sph)) return rc;
    if (int rc = upload(s->d_msph, msph, &d.msph)) return rc;
    if (int rc = upload(s->d_rect, rect, &d.rect)) return rc;
    if (int rc = upload(s->d_groups, groups, &d.groups)) return rc;
    if (int rc = upload(s->d_bez, bez, &d.bez)) return rc;
    d.n_bez = (int)bez.size();
    if (int rc = upload(s->d_klein, klein, &d.klein)) return rc;
    d.n_klein = (int)klein.size();
    if (int rc = upload(s->d_med, med, &d.med)) return rc;
    d.n_med = (int)med.size();
    if (int rc = upload(s->d_bgroups, bgroups, &d.bgroups)) return rc;
    d.n_bgroups = (int)bgroups.size();
    d.bvh_has_bez = bvh_has_bez ? 1 : 0;
    d.bez_groups = 0;
    for (const Group& G : groups) d.bez_groups += G.type == LEAF_BEZIER ? 1 : 0;
    d.bvh_pad = bvh_pad;
    if (int rc = upload(s->d_bvh2, bvh2, &d.bvh2)) return rc;
    if (int rc = upload(s->d_bleaf, bleaf, &d.bleaf)) return rc;
    d.n_bvh2 = (int)bvh2.size();
    d.bvh2_root = bvh2_root;
    if (!fbvh2.empty()) {
        std::vector<int32_t> fid;
        for (const auto& sl : fsrc) fid.push_back(base[sl.first] + sl.second);
        if (int rc = upload(s->d_fbvh2, fbvh2, &d.fbvh2)) return rc;
        if (int rc = upload(s->d_fbleaf, fbleaf, &d.fbleaf)) return rc;
        if (int rc = upload(s->d_fsph, fsph, &d.fsph)) return rc;
        if (int rc = upload(s->d_fid, fid, &d.fid)) return rc;
        d.fbvh2_root = fbvh2_root;
        d.n_fbvh2 = (int)fbvh2.size(); d.n_fbleaf = (int)fbleaf.size(); d.n_fsph = (int)fsph.size();
        d.tree0_any_time = tree0_any_time ? 1 : 0;
    }
    d.n_bleaf = (int)bleaf.size();
    d.lane_stack = lane_stack;
    if (lane_stack > kLaneStack) return fail("internal: BVH deeper than the traversal stack");
    if (!bvh4.empty()) {
        if (int rc = upload(s->d_bvh4, bvh4, &d.bvh4)) return rc;
        d.n_bvh4 = (int)bvh4.size();
        d.bvh4_root = bvh4_root;
        d.stack4 = stack4;
        // the walk's LDS stack column: kCurveLdsStack entries (a walk rarely holds more; the rest go to the
        // overflow area), so the curve kernel's blocks stay small.  RTAMD_CURVE_LDS_STACK (tests): fewer
        // entries, so the walk exercises its overflow area
        const char* ce = std::getenv("RTAMD_CURVE_LDS_STACK");
        d.lds4 = std::min(lane_stack, ce ? std::max(1, std::atoi(ce)) : kCurveLdsStack);
        {                                            // survivor rings: kCurveWaves 256-thread blocks per CU
            int dev = 0, cus = 0;
            HIPCHK(hipGetDevice(&dev));
            HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            d.ring_waves = (uint32_t)std::max(cus, 1) * 4u * (uint32_t)kCurveWaves;
            HIPCHK(s->d_bez_ring.ensure((size_t)kLanes * d.ring_waves * kBezRing * 128u));
            d.bez_ring = s->d_bez_ring.as<double>();
            HIPCHK(s->d_fuse_ring.ensure((size_t)kLanes * d.ring_waves * kFuseWaveBytes));
            d.fuse_ring = s->d_fuse_ring.as<uint8_t>();
        }
        if (stack4 > d.lds4) {                       // the walk's deepest stacks spill past the LDS columns
            int dev = 0, cus = 0;
            HIPCHK(hipGetDevice(&dev));
            HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            d.ovf_lanes = (uint32_t)std::max(cus, 1) * 2048u;     // any resident grid of 256-thread blocks
            HIPCHK(s->d_stk_ovf.ensure((size_t)kLanes * d.ovf_lanes * (size_t)(stack4 - d.lds4) * sizeof(uint32_t)));
            d.stk_ovf = s->d_stk_ovf.as<uint32_t>();
        }
    }
    if (int rc = upload(s->d_chains, chains, &d.chains)) return rc;
    if (int rc = upload(s->d_leaves, leaves, &d.leaves)) return rc;
    {
        std::vector<uint8_t> lc((leaves.size() + 15) / 16 * 16 + 16, 0);
        for (size_t k = 0; k < leaves.size(); ++k) lc[k] = (uint8_t)leaves[k].mtype;
        if (int rc = upload(s->d_leaf_cls, lc, &d.leaf_cls)) return rc;
    }
    {   // the world's leaf ids in list order (list_closest); none for scenes with media, which keep the grouped scan
        std::vector<int32_t> order;
        if (med.empty()) {
            order.reserve(f.leaves.size());
            for (size_t i = 0; i < f.leaves.size(); ++i)
                if (ord_type[i] >= 0) order.push_back(base[ord_type[i]] + ord_local[i]);
            if (order.size() != leaves.size()) return fail("internal: list order and leaf records out of step");
        }
        if (int rc = upload(s->d_order, order, &d.order)) return rc;
        d.n_order = (int32_t)order.size();
        if (generic) {                               // leaf ids of the tree leaves, and every leaf's list position
            std::vector<int32_t> gleaf, pos(leaves.size(), 0);
            gleaf.reserve(gsrc.size());
            for (const auto& tl : gsrc) gleaf.push_back(base[tl.first] + tl.second);
            for (size_t k = 0; k < order.size(); ++k) pos[(size_t)order[k]] = (int32_t)k;
            if (int rc = upload(s->d_gleaf, gleaf, &d.gleaf)) return rc;
            d.n_gleaf = (int32_t)gleaf.size();
            if (int rc = upload(s->d_leaf_pos, pos, &d.leaf_pos)) return rc;
            if (int rc = upload(s->d_rot, rot, &d.rot)) return rc;
            d.n_rot = (int32_t)rot.size();
            if (!g0bvh2.empty() || !g0bleaf.empty()) {
                if (int rc = upload(s->d_g0bvh2, g0bvh2, &d.g0bvh2)) return rc;
                if (int rc = upload(s->d_g0bleaf, g0bleaf, &d.g0bleaf)) return rc;
                d.g0bvh2_root = g0bvh2_root;
                d.n_g0bvh2 = (int32_t)g0bvh2.size();
            }
        }
    }
    {   // rt_get_tree_info
        rt_tree_info& ti = s->tree;
        std::memset(&ti, 0, sizeof ti);
        if (use_bvh) {
            for (const PrimRef& r : refs) {
                const bool world = f.leaves[(size_t)r.leaf].chain == -1;
                if (r.type == LEAF_BEZIER) ++ti.curve_leaves;
                else if (world && (r.type == LEAF_SPHERE || r.type == LEAF_MSPHERE)) ++ti.sphere_leaves;
                else ++ti.generic_leaves;
            }
            ti.nodes = (int32_t)bvh2.size(); ti.depth = depth_all;
            ti.nodes0 = (int32_t)(generic ? g0bvh2.size() : fbvh2.size()); ti.depth0 = depth0;
        }
        ti.group_leaves = (int32_t)leaves.size() - ti.sphere_leaves - ti.curve_leaves - ti.generic_leaves;
        ti.rot_entries = generic ? (int32_t)rot.size() : 0;
        ti.generic_min = (int32_t)gen_min;
    }
    if (int rc = upload(s->d_mats, s->mats, &d.mats)) return rc;
    if (int rc = upload(s->d_texs, s->texs, &d.texs)) return rc;
    d.n_sph = (int)sph.size(); d.n_msph = (int)msph.size(); d.n_rect = (int)rect.size();
    d.n_groups = (int)groups.size(); d.n_chains = (int)chains.size(); d.n_leaves = (int)leaves.size();
    d.msph_shared = 0;
    if (!msph.empty()) {
        bool same = true;
        for (const MSphereRec& m : msph)
            same = same && std::memcmp(&m.t0, &msph[0].t0, sizeof(double)) == 0 &&
                   std::memcmp(&m.den, &msph[0].den, sizeof(double)) == 0;
        if (same) { d.msph_shared = 1; d.msph_t0 = msph[0].t0; d.msph_den = msph[0].den; }
    }
    d.bvh_solo = (groups.size() == 1 && groups[0].type == GROUP_BVH && !bvh_has_bez && tree0_direct &&
                  !std::getenv("RTAMD_NO_SOLO")) ? 1 : 0;
    d.n_mats = (int)s->mats.size(); d.n_texs = (int)s->texs.size();
    for (int k = 0; k < kLeafTypes; ++k) d.leaf_base[k] = base[k];
    d.has_perlin = s->have_perlin ? 1 : 0;
    d.has_noise_tex = 0;
    for (const auto& t : s->texs) if (t.type == TEX_NOISE || t.type == TEX_MARBLE) d.has_noise_tex = 1;
    d.has_image_tex = 0;
    for (const auto& t : s->texs) if (t.type == TEX_IMAGE) d.has_image_tex = 1;
    if (d.has_image_tex) {
        if (int rc = upload(s->d_teximg, s->teximg, &d.teximg)) return rc;
    }
    if (s->have_perlin) {
        if (int rc = upload(s->d_ranvec, s->ranvec, &d.ranvec)) return rc;
        if (int rc = upload(s->d_perm, s->perm, &d.perm)) return rc;
    }
    d.sky = s->sky;
    std::memset(&d.light, 0, sizeof d.light);
    if (s->light >= 0) {
        const Obj* L = &s->objs[s->light];
        while (L->type == O_FLIP) L = &s->objs[L->child];
        if (L->type == O_RECT) {
            d.light.type = LIGHT_RECT; d.light.axis = L->axis;
            d.light.a0 = L->a0; d.light.a1 = L->a1; d.light.b0 = L->b0; d.light.b1 = L->b1; d.light.k = L->k;
        } else {
            d.light.type = LIGHT_SPHERE;
            d.light.cx = L->c0[0]; d.light.cy = L->c0[1]; d.light.cz = L->c0[2]; d.light.r = L->r;
        }
    }
    d.mat_mask = 0;
    for (const auto& m : s->mats) d.mat_mask |= 1 << m.type;
    const double* cm = s->cam;
    for (int k = 0; k < 3; ++k) {
        d.cam.llc[k] = cm[k]; d.cam.hor[k] = cm[3 + k]; d.cam.ver[k] = cm[6 + k];
        d.cam.origin[k] = cm[9 + k]; d.cam.w[k] = cm[12 + k]; d.cam.u[k] = cm[15 + k]; d.cam.v[k] = cm[18 + k];
    }
    d.cam.lens = cm[21]; d.cam.t0 = cm[22]; d.cam.t1 = cm[23];
    for (const Obj& o : s->objs)
        if (o.mat >= (int)s->mats.size()) return fail("object refers to an unknown material");
    // LDS footprints of the persistent kernels: only now is every count and
    // the stack depth in `d` final (the kernels carve their LDS from the same fields)
    s->ext_lds = 0;
    s->ext_lds_blocks = 0;
    if (!std::getenv("RTAMD_NO_EXTEND_LDS")) {
        const size_t lds = extend_lds_bytes(d);
        uint32_t mb = 0;
        if (lds > 0 && lds <= extend_lds_budget() && extend_lds_prepare(d, lds, &mb) == hipSuccess && mb >= 256) {
            s->ext_lds = lds;
            s->ext_lds_blocks = mb;           // every resident block (50-88 % of them: -0.3 .. -3 %, profiles/r02/pct)
        }
        (void)hipGetLastError();
    }
    s->cam_lds = 0;
    s->cam_blocks = 0;
    if (!std::getenv("RTAMD_NO_CAMERA_LDS")) {
        const size_t lds = camera_lds_bytes(d);
        uint32_t mb = 0;
        if (lds > 0 && lds <= extend_lds_budget() && camera_prepare(d, lds, &mb) == hipSuccess && mb >= 256) {
            s->cam_lds = lds;
            s->cam_blocks = mb;
        }
        (void)hipGetLastError();
    }
    HIPCHK(s->d_dev.ensure(sizeof(DevScene)));
    COMMIT_MARK("upload");
    HIPCHK(hipMemcpy(s->d_dev.p, &d, sizeof(DevScene), hipMemcpyHostToDevice));
    s->committed = true;
    g_reaper.reap(std::move(f), std::move(refs), std::move(bvh_nodes), std::move(bvh2), std::move(bleaf), std::move(bvh4),
                  std::move(sph), std::move(msph), std::move(bez), std::move(lsph), std::move(lmsph), std::move(lbez),
                  std::move(leaves), std::move(fbvh2), std::move(fbleaf), std::move(fsph));
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
