// Host engine + C ABI (include/gpudrive_amd.h).  Citations are relative to the reference checkout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <atomic>
#include <exception>
#include <string>
#include <thread>
#include <vector>

#include "dev_mem.hpp"
#include "engine.hpp"
#include "gd_math.hpp"
#include "scene.hpp"
#ifdef GD_CLOCKS
namespace gd { void set_clocks_read(unsigned long long *out); void step_clocks_read(unsigned long long *out); }
#endif
#ifndef GD_GRID_MIN_CELL
#define GD_GRID_MIN_CELL 16.f
#endif

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIP_CHECK(expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            throw HipError(std::string(#expr) + " failed: " + hipGetErrorString(e_));               \
    } while (0)

struct TensorSpec {
    int dtype;
    int ndim;
    int64_t dims[5];
};

TensorSpec tensor_spec(int id, int64_t W, int64_t A) {
    switch (id) {
    case GD_T_ACTION: return {GD_DTYPE_F32, 3, {W, A, 10}};
    case GD_T_REWARD: return {GD_DTYPE_F32, 3, {W, A, 1}};
    case GD_T_DONE: return {GD_DTYPE_I32, 3, {W, A, 1}};
    case GD_T_INFO: return {GD_DTYPE_I32, 3, {W, A, 5}};
    case GD_T_SELF_OBS: return {GD_DTYPE_F32, 3, {W, A, 8}};
    case GD_T_ABS_OBS: return {GD_DTYPE_F32, 3, {W, A, 14}};
    case GD_T_PARTNER_OBS: return {GD_DTYPE_F32, 4, {W, A, A - 1, 9}};
    case GD_T_AGENT_MAP_OBS: return {GD_DTYPE_F32, 4, {W, A, GD_MAP_OBS_K, 9}};
    case GD_T_MAP_OBS: return {GD_DTYPE_F32, 3, {W, GD_MAX_ROAD_ENTITIES, 9}};
    case GD_T_LIDAR: return {GD_DTYPE_F32, 5, {W, A, 3, GD_NUM_LIDAR_SAMPLES, 4}};
    case GD_T_BEV: return {GD_DTYPE_F32, 5, {W, A, GD_BEV_RES, GD_BEV_RES, 1}};
    case GD_T_STEPS_REMAINING: return {GD_DTYPE_I32, 3, {W, A, 1}};
    case GD_T_SHAPE: return {GD_DTYPE_I32, 2, {W, 2}};
    case GD_T_CONTROLLED_STATE: return {GD_DTYPE_I32, 3, {W, A, 1}};
    case GD_T_RESPONSE_TYPE: return {GD_DTYPE_I32, 3, {W, A, 1}};
    case GD_T_EXPERT_TRAJECTORY: return {GD_DTYPE_F32, 3, {W, A, GD_TRAJECTORY_FLOATS}};
    case GD_T_WORLD_MEANS: return {GD_DTYPE_F32, 2, {W, 3}};
    case GD_T_METADATA: return {GD_DTYPE_I32, 3, {W, A, 4}};
    case GD_T_DELETED_AGENTS: return {GD_DTYPE_I32, 2, {W, A}};
    case GD_T_MAP_NAME: return {GD_DTYPE_I32, 2, {W, 32}};
    case GD_T_SCENARIO_ID: return {GD_DTYPE_I32, 2, {W, 32}};
    }
    return {-1, 0, {0}};
}

int64_t spec_bytes(const TensorSpec &s) {
    int64_t n = 4;
    for (int i = 0; i < s.ndim; i++) n *= s.dims[i];
    return n;
}

// runtime handles that destroy themselves (hipEvent_t and hipStream_t are pointers to opaque structs)
struct HandleDelete {
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
    void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
    void operator()(int32_t *pinned) const { (void)hipHostFree(pinned); }
};
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, HandleDelete>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, HandleDelete>;
using PinnedFlags = std::unique_ptr<int32_t, HandleDelete>;

Event make_event(unsigned flags = hipEventDefault) {
    hipEvent_t e = nullptr;
    HIP_CHECK(hipEventCreateWithFlags(&e, flags));
    return Event(e);
}

struct EventPair {
    Event start, stop;
};

// What rebuild_worlds keeps of one world on the host, to repack the batch's arrays on set_maps / deleteAgents.
struct WorldHost {
    std::vector<float> xy, aux;    // road points, road records
    int agents = 0;                // live agents (shape[w][0])
    std::vector<int32_t> resp;     // response type of every agent slot (who can move at all)
    std::vector<gd::RoadBox> boxes;
    gd::GridHdr grid{};            // grid over the collidable boxes
    std::vector<int32_t> cell_off, cell_items;
    gd::GridHdr rgrid{};           // grid over all roads (set-order selection)
    std::vector<int32_t> rcell_off;
    std::vector<uint16_t> rcell_items;
};

// A device array of T that rebuild_worlds may have to grow: n entries are written and kReadable more must exist behind them;
// when that does not fit, the array is reallocated (contents gone) with room for n + n / 8 + kPad.
struct Float8 { float v[8]; };
template <typename T, size_t kReadable, size_t kPad>
struct Growable {
    gd::DevMem mem;
    // `view` is the kernels' pointer to the array: written here, so that it never holds an address that was returned (null
    // while the owner is empty, i.e. when the allocation threw).  True when the array was reallocated.
    template <typename V>
    bool fit(size_t n, V *&view) {
        view = nullptr;
        const bool grew = mem.reserve((n + kReadable) * sizeof(T), (n + n / 8 + kPad) * sizeof(T));
        view = static_cast<V *>(mem.get());
        return grew;
    }
    void upload(const void *src, size_t n) const {
        if (n) HIP_CHECK(hipMemcpy(mem.get(), src, n * sizeof(T), hipMemcpyHostToDevice));
    }
};

}  // namespace

// dev_mem.hpp's two hooks
void *gd::dev_alloc(size_t bytes) {
    void *p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes));
    return p;
}
void gd::dev_free(void *p) noexcept { (void)hipFree(p); }

struct gd_sim {
    gd_config cfg{};
    gd_params params{};
    int W = 0, A = 0;
    hipStream_t stream = nullptr;
    gd::DevSim d{};
    // Members are declared so that what is left after ~gd_sim's synchronise may go in any order: device memory, pinned
    // memory, events and the side stream each return themselves.
    void *exported[GD_T_COUNT] = {};        // views: the engine's own tensors (exported_mem) or the caller's (borrowed)
    gd::DevMem exported_mem[GD_T_COUNT];
    std::vector<gd::DevMem> internal;       // fixed-size arrays, allocated once (alloc_internal)
    std::vector<std::string> scenes;
    std::vector<int32_t> deleted;  // host mirror [W][A]
    std::vector<WorldHost> world_host;  // per-world host road data (kept to repack the CSR on set_maps / deleteAgents)
    int cu_count = 256;
    // The arrays a rebuild may grow, each with its rule: <entry, readable entries behind the last one, padding>.
    // k_map_obs requests chunks of 32 roads up to 256 roads past a world's last one, and the fused set-order write-out
    // reads road_rec[first road of the world] even for a world without roads: the road arrays always end in 320 readable
    // pad entries (also when a rebuild fits the old capacity, and when no world has a road)
    Growable<float2, 320, 640> road_xy;
    Growable<Float8, 320, 640> road_aux, road_rec;
    Growable<gd::RoadBox, 0, 64> boxes;
    Growable<int32_t, 0, 64> cell_off, cell_items;
    Growable<float4, 0, 64> cell_hdr;
    Growable<int32_t, 0, 64> rcell_off;
    Growable<uint16_t, 64, 128> rcell_items, rcell_pos;
    Growable<float2, 64, 128> rcell_xy;
    Growable<float4, 0, 64> road_blk;
    // per-world tables the engine uploads and the kernels only read (DevSim holds const views of them)
    int32_t *d_road_off = nullptr, *d_box_off = nullptr, *d_blk_off = nullptr;
    gd::GridHdr *d_grid = nullptr, *d_rgrid = nullptr;
    float4 *d_road_bbox = nullptr;
    float *d_road_rbmax = nullptr;
    // pinned flag staging ring
    static constexpr int kRing = 8;
    PinnedFlags h_flags[kRing];
    Event flag_ev[kRing];
    int ring_pos = 0;
    // kernel timing
    // A fixed ring of event pairs per kernel, created when timing is switched on: a launch re-records the oldest pair
    // after its elapsed time has been read.  (Round 2 kept one pair per launch alive until the read-out; the runtime's
    // signal pool then ran dry in the middle of a timed stretch and one hipLaunchKernel blocked the host for 14 ms --
    // tools/trace_gap.sh -- so that a 20-step wall clock was far above the sum of its kernels.)
    static constexpr size_t kEvRing = 32;
    // second stream for the partner rows (k_partner_rows beside the road kernels): forked and joined with events, also
    // inside the captured step graph
    Stream side;
    Event ev_fork, ev_join;
    size_t lin_cap = 0;        // entries of d.lin_list / d.lin_list_dyn
    // learner rows (gd_set_learner_rows): both maps, [W * A] each, and the row count the map kernel returns; d.row_of_slot /
    // d.slot_of_row point at them while rows are set
    int32_t *d_row_of_slot = nullptr, *d_slot_of_row = nullptr, *d_row_count = nullptr;
    int32_t *d_lin_list = nullptr, *d_lin_list_dyn = nullptr;
    bool full_pass_next = false;  // the next step's road pass takes every live agent (state was written from outside)
    int64_t lin_static_agents = 0;   // live agents that are not on the step passes' list (response type Static)
    int64_t host_skipped = 0;        // ... counted as left in place once per step pass (gd_stat 30 adds the device's counters)
    bool rk_possible = false;  // reference order, k-NN, not switched off: a batch may take the rank replay
    bool rk_alloc = false;     // its buffers exist

    // 4.7 KB per agent slot for ALL W * A slots (0.31 GB at 1024 x 64, 1.2 GB at 4096 x 64), allocated when a batch first takes
    // the rank replay and kept for the life of the simulator.  The path is a scheduling choice, never a result: when the
    // device cannot give the memory, what was allocated is returned, the batch stays on k_map_obs (same rows) and the
    // rank replay is not tried again for this simulator.
    bool ensure_rank_buffers() {
        if (rk_alloc) return true;
        const size_t WA = static_cast<size_t>(W) * A;
        // into local owners and a local copy of the kernels' view: published together when every allocation succeeded
        std::vector<gd::DevMem> mine;
        gd::DevSim n = d;
        try {
            alloc_into(mine, n.rk_E, WA * GD_RANK_CAP + 64);  // the replay prefetches up to 24 entries past a row
            alloc_into(mine, n.rk_spc, WA * GD_RANK_SPL);
            // developer switch for the test of the path below: the device "runs out of memory" in the middle of the allocations
            if (std::getenv("GPUDRIVE_RANK_ALLOC_FAIL") != nullptr)
                throw HipError("GPUDRIVE_RANK_ALLOC_FAIL: simulated allocation failure of the rank replay's buffers");
            alloc_into(mine, n.rk_kt, WA * GD_RANK_KT);
            alloc_into(mine, n.rk_heap, WA * GD_RANK_HEAP_DW);
            alloc_into(mine, n.rk_cpe, WA * GD_RANK_NCP);
            alloc_into(mine, n.rk_n, WA);
            alloc_into(mine, n.rk_fallback, WA / 32);
            alloc_into(mine, n.rk_streak, WA / 32);
            alloc_into(mine, n.cp_road, 2 * WA * GD_RANK_NCP);
            alloc_into(mine, n.cp_T, 2 * WA * GD_RANK_NCP);
            alloc_into(mine, n.cp_hdr, 2 * WA);
            alloc_into(mine, n.rk_cpf, WA * GD_RANK_NCP);
            alloc_into(mine, n.rk_cpt, WA * GD_RANK_NCP);
            alloc_into(mine, n.rk_rec, WA);
            alloc_into(mine, n.rk_hist, GD_RH_ALLOC);
            alloc_into(mine, n.rk_ticket, WA);
            alloc_into(mine, n.rk_order, WA);
            alloc_into(mine, n.rk_list, 8 * WA);
            // the long list: room for a quarter of the agent slots (an agent beyond that takes the fallback)
            n.rk_nlong = static_cast<int>(std::max<size_t>(WA / 4, 64));
            alloc_into(mine, n.rk_longlist, n.rk_nlong);
            alloc_into(mine, n.rk_longslot, WA);
            alloc_into(mine, n.rk_E_long, static_cast<size_t>(n.rk_nlong) * GD_RANK_CAP_LONG + 64);  // (+ the replay's prefetch)
            alloc_into(mine, n.rk_kt_long, static_cast<size_t>(n.rk_nlong) * GD_RANK_KT_LONG);
            internal.reserve(internal.size() + mine.size());
        } catch (const HipError &) {  // `mine` returns what was allocated; d never saw it
            (void)hipGetLastError();
            rk_possible = false;
            d.rk_on = 0;
            return false;
        }
        for (gd::DevMem &m : mine) internal.push_back(std::move(m));
        d = n;
        rk_alloc = true;
        return true;
    }
    bool timing = false;
    std::vector<EventPair> ev_pool[gd::KERNEL_TIMED];
    size_t ev_head[gd::KERNEL_TIMED] = {};  // oldest recorded pair
    size_t ev_used[gd::KERNEL_TIMED] = {};  // recorded pairs not read yet
    double ev_ms[gd::KERNEL_TIMED] = {};
    int64_t ev_launches[gd::KERNEL_TIMED] = {};

    ~gd_sim() {  // what is about order: nothing returns itself while the device still works, and the graph goes first
        (void)hipDeviceSynchronize();
        if (step_graph) (void)hipGraphExecDestroy(step_graph);
    }

    // a zero-filled array of `count` T (at least 16 bytes), owned by `into`
    template <typename T>
    static void alloc_into(std::vector<gd::DevMem> &into, T *&field, size_t count) {
        const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
        into.emplace_back(bytes);  // owned from here on: a failing memset must not leak it
        HIP_CHECK(hipMemset(into.back().get(), 0, bytes));
        field = static_cast<T *>(into.back().get());
    }
    template <typename T>
    T *alloc_internal(size_t count) {
        T *p = nullptr;
        alloc_into(internal, p, count);
        return p;
    }

    void collect_timing(int k, size_t keep = 0) {  // read the oldest pairs until `keep` are left
        while (ev_used[k] > keep) {
            const EventPair &e = ev_pool[k][ev_head[k]];
            float ms = 0.f;
            if (hipEventSynchronize(e.stop.get()) == hipSuccess && hipEventElapsedTime(&ms, e.start.get(), e.stop.get()) == hipSuccess) {
                ev_ms[k] += ms;
                ev_launches[k]++;
            }
            ev_head[k] = (ev_head[k] + 1) % ev_pool[k].size();
            ev_used[k]--;
        }
    }

    void launch(int which, bool move, hipStream_t stream_override = nullptr) {
        hipStream_t stream = stream_override ? stream_override : this->stream;
        const bool timed = timing && which < gd::KERNEL_TIMED && !d.gate_any;  // gated reset passes are mostly empty launches
        const EventPair *ep = nullptr;
        if (timed) {
            // ring full: read the older half (those launches finished long ago; the host stays well ahead of the GPU)
            if (ev_used[which] == ev_pool[which].size()) collect_timing(which, ev_pool[which].size() / 2);
            ep = &ev_pool[which][(ev_head[which] + ev_used[which]) % ev_pool[which].size()];
            ev_used[which]++;
            HIP_CHECK(hipEventRecord(ep->start.get(), stream));
        }
        if (which == gd::KERNEL_BEV) gd::launch_bev(d, stream);
        else if (which == gd::KERNEL_LIDAR) gd::launch_lidar(d, stream);
        else gd::launch_kernel(d, stream, which, move);
        if (timed) HIP_CHECK(hipEventRecord(ep->stop.get(), stream));
        HIP_CHECK(hipGetLastError());
    }

    // The Step task graph as one hipGraph: the kernels of a step are captured once on the engine's
    // stream and replayed with a single hipGraphLaunch (the kernel arguments are the DevSim struct by
    // value, so any change of it -- rebuilt worlds, a new stream, timing mode -- drops the graph).
    hipGraphExec_t step_graph = nullptr;
    int64_t stat_graph_steps = 0, stat_plain_steps = 0, stat_captures = 0;
    bool graph_ok = std::getenv("GPUDRIVE_NO_GRAPH") == nullptr;

    void drop_graph() {
        if (step_graph) {
            (void)hipGraphExecDestroy(step_graph);
            step_graph = nullptr;
        }
    }

    // Set-order road kernel: how the agents are dealt to workgroups and which of its two equivalent write-outs runs
    // (map_obs.hip, launch_map_obs).  Neither changes a result.  Measured (road observation, us; tools/set_schedules.sh),
    // agents per wave 1 / 2 / 4 / 16:
    //   1024 full worlds (synthetic)   row kernel 183 / 181 / 180 / 192     fused 181 / 168 / 167 / 167
    //   1024 ragged worlds (Waymo)     row kernel  83 /  80 /  82 /  84     fused  61 /  70 /  67 /  80
    //   4096 ragged worlds             row kernel 411 / 399 / 392 / 392     fused 249 / 246 / 256 / 274
    // Rounds 2 and 3 chose by batch shape (row kernel for full worlds, sixteen agents per wave for thousands of worlds):
    // the selection then took twice the instructions it takes now (map_obs.hip), and rows stored by the selecting waves
    // had little to hide behind.  Now: always fused, two agents per wave -- enough workgroups for every batch, and the
    // second agent's inputs arrive while the first is selected.
    // GPUDRIVE_SET_FUSED_ROWS=0|1 and GPUDRIVE_SET_AGENTS_PER_WAVE=n pin them (the tests run the combinations).
    void choose_set_schedule() {
        d.set_apw = 2;
        d.set_fused_rows = 1;
        if (const char *e = std::getenv("GPUDRIVE_SET_FUSED_ROWS")) d.set_fused_rows = std::atoi(e) != 0 ? 1 : 0;
        if (const char *e = std::getenv("GPUDRIVE_SET_AGENTS_PER_WAVE")) d.set_apw = std::min(32, std::max(1, std::atoi(e)));
    }

    void step() {
        if (full_pass_next) {  // (gd_debug_set_state moved agents behind the engine's back: nobody is left out of this step's road pass / rasters)
            full_pass_next = false;
            d.lin_dyn_off = 1;
            d.bev_all_dirty = 1;
            try {
                run_rest(true);
            } catch (...) {
                d.lin_dyn_off = 0;
                d.bev_all_dirty = 0;
                throw;
            }
            d.lin_dyn_off = 0;
            d.bev_all_dirty = 0;
            stat_plain_steps++;
            return;
        }
        // (the agents a linear step pass does not even visit are agents whose rows are left in place)
        if (params.roadObservationAlgorithm != GD_ROADS_K_NEAREST && d.lin_on && d.pose_skip && !params.disableClassicalObs)
            host_skipped += lin_static_agents;
        if (!graph_ok || timing || stream == nullptr) {  // the legacy null stream cannot be captured
            run_rest(true);
            stat_plain_steps++;
            return;
        }
        if (!step_graph) {
            hipGraph_t g = nullptr;
            if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
                (void)hipGetLastError();
                graph_ok = false;
                run_rest(true);
                return;
            }
            try {
                run_rest(true);
            } catch (...) {
                (void)hipStreamEndCapture(stream, &g);
                if (g) (void)hipGraphDestroy(g);
                throw;
            }
            HIP_CHECK(hipStreamEndCapture(stream, &g));
            stat_captures++;
            const hipError_t e = hipGraphInstantiate(&step_graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (e != hipSuccess) {  // fall back to plain launches for good
                step_graph = nullptr;
                graph_ok = false;
                run_rest(true);
                return;
            }
        }
        HIP_CHECK(hipGraphLaunch(step_graph, stream));
        stat_graph_steps++;
    }

    // setupRestOfTasks, src/sim.cpp:785-943
    void run_rest(bool move) {
        launch(gd::KERNEL_STATE, move);
        // GPUDRIVE_SPLIT_PARTNER=1 (off by default): the partner rows (148 MB of stores at 1024 x 64, nothing downstream of
        // them in the step) on the second stream, beside the road kernels; joined before anything else of the caller's
        // stream can follow.  Measured SLOWER in every workload (step, ms: synthetic 1.48 vs 1.42, Waymo tiles 0.68 vs
        // 0.53, set order 0.43 vs 0.40): beside the road kernels the row kernel takes 86-273 us instead of 28 and the step
        // waits for it at the join.
        const bool fork = d.split_partner && !params.disableClassicalObs;
        if (fork) {
            HIP_CHECK(hipEventRecord(ev_fork.get(), stream));
            HIP_CHECK(hipStreamWaitEvent(side.get(), ev_fork.get(), 0));
            launch(gd::KERNEL_PARTNER, move, side.get());
            HIP_CHECK(hipEventRecord(ev_join.get(), side.get()));
        }
        if (!params.disableClassicalObs) launch(gd::KERNEL_MAP_OBS, move);
        if (!params.disableClassicalObs && d.bev) {  // collectBevObservationsSystem, src/sim.cpp:879-884 (opt-in)
            launch(gd::KERNEL_BEV, move);
        }
        if (params.enableLidar) {  // lidarSystem, src/sim.cpp:895-913
            launch(gd::KERNEL_LIDAR, move);
        }
        if (fork) HIP_CHECK(hipStreamWaitEvent(stream, ev_join.get(), 0));
    }

    void upload_flags(int32_t *dst, const std::vector<int32_t> &flags) {
        const int slot = ring_pos;
        ring_pos = (ring_pos + 1) % kRing;
        HIP_CHECK(hipEventSynchronize(flag_ev[slot].get()));
        std::memcpy(h_flags[slot].get(), flags.data(), sizeof(int32_t) * W);
        HIP_CHECK(hipMemcpyAsync(dst, h_flags[slot].get(), sizeof(int32_t) * W, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipEventRecord(flag_ev[slot].get(), stream));
    }

    // (Re)build the listed worlds on the host and upload their init-time rows:
    // MapReader::parseAndWriteOut + createPersistentEntities (src/mgr.cpp:527-535,630-647;
    // src/level_gen.cpp:396-465).
    void rebuild_worlds(const std::vector<int> &worlds) {
        HIP_CHECK(hipStreamSynchronize(stream));
        drop_graph();
        std::map<std::string, std::shared_ptr<const gd::SceneMap>> scene_cache;
        std::map<std::string, std::shared_ptr<gd::HostWorld>> world_cache;
        std::vector<int32_t> rebuilt(W, 0);
        // Worlds are staged in runs of consecutive indices (at most kRun) so that every tensor slice of
        // a run goes up in ONE copy: 1024 worlds need ~150 hipMemcpy calls instead of ~20 per world.
        constexpr int kRun = 128;
        std::vector<int> sorted_worlds(worlds);
        std::sort(sorted_worlds.begin(), sorted_worlds.end());
        struct Staging {
            std::vector<float> traj, map_obs, planes[7], means;
            std::vector<int32_t> etype, agent_id, resp, controlled, metadata, deleted, map_name, scenario_id, shape;
        } st;
        auto flush = [&](int w0, int nw) {
            if (nw == 0) return;
            const size_t o = static_cast<size_t>(w0) * A;
            auto up = [&](void *dst, const void *src, size_t bytes) {
                HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
            };
            up(d.traj + o * GD_TRAJECTORY_FLOATS, st.traj.data(), st.traj.size() * 4);
            up(d.map_obs + static_cast<size_t>(w0) * GD_MAX_ROAD_ENTITIES * 9, st.map_obs.data(), st.map_obs.size() * 4);
            float *planes[7] = {d.len, d.wid, d.hgt, d.sc0, d.sc1, d.goal_x, d.goal_y};
            for (int k = 0; k < 7; k++) up(planes[k] + o, st.planes[k].data(), st.planes[k].size() * 4);
            up(d.etype + o, st.etype.data(), st.etype.size() * 4);
            up(d.agent_id + o, st.agent_id.data(), st.agent_id.size() * 4);
            up(d.resp + o, st.resp.data(), st.resp.size() * 4);
            up(d.controlled + o, st.controlled.data(), st.controlled.size() * 4);
            up(d.metadata + o * 4, st.metadata.data(), st.metadata.size() * 4);
            up(d.deleted + o, st.deleted.data(), st.deleted.size() * 4);
            up(d.means + static_cast<size_t>(w0) * 3, st.means.data(), st.means.size() * 4);
            up(d.map_name + static_cast<size_t>(w0) * 32, st.map_name.data(), st.map_name.size() * 4);
            up(d.scenario_id + static_cast<size_t>(w0) * 32, st.scenario_id.data(), st.scenario_id.size() * 4);
            up(d.shape + static_cast<size_t>(w0) * 2, st.shape.data(), st.shape.size() * 4);
            st = Staging();
        };
        // Parse the distinct scenes of this call on a few host threads first: MapReader::parseAndWriteOut runs
        // on ONE thread per set_maps in the reference (src/mgr.cpp:630-647), ~9 ms of JSON per scene here.
        {
            std::vector<std::string> todo;
            for (int w : sorted_worlds)
                if (scene_cache.emplace(scenes[w], nullptr).second) todo.push_back(scenes[w]);
            std::vector<std::shared_ptr<const gd::SceneMap>> parsed(todo.size());
            std::vector<std::exception_ptr> errors(todo.size());
            const unsigned hc = std::thread::hardware_concurrency();
            const size_t nthreads = std::min<size_t>(todo.size(), std::min<size_t>(16, hc ? hc : 1));
            std::atomic<size_t> next{0};
            auto worker = [&]() {
                for (size_t k; (k = next.fetch_add(1)) < todo.size();) {
                    try {
                        parsed[k] = gd::load_scene(todo[k], params.polylineReductionThreshold);
                    } catch (...) {
                        errors[k] = std::current_exception();
                    }
                }
            };
            std::vector<std::thread> pool;
            for (size_t t = 1; t < nthreads; t++) pool.emplace_back(worker);
            worker();
            for (auto &t : pool) t.join();
            for (size_t k = 0; k < todo.size(); k++) {
                if (errors[k]) std::rethrow_exception(errors[k]);  // first failing scene in world order
                scene_cache[todo[k]] = parsed[k];
            }
        }
        int run_start = -1, run_len = 0;
        for (int w : sorted_worlds) {
            if (run_len > 0 && (w != run_start + run_len || run_len == kRun)) {
                flush(run_start, run_len);
                run_len = 0;
            }
            if (run_len == 0) run_start = w;
            run_len++;
            const std::string &path = scenes[w];
            const int32_t *del = deleted.data() + static_cast<size_t>(w) * A;
            int ndel = 0;
            std::string key = path;
            for (int i = 0; i < A; i++)
                if (del[i] != -1) { ndel = i + 1; }
            for (int i = 0; i < ndel; i++) key += "|" + std::to_string(del[i]);
            std::shared_ptr<gd::HostWorld> hw;
            auto it = world_cache.find(key);
            if (it != world_cache.end()) {
                hw = it->second;
            } else {
                auto sit = scene_cache.find(path);  // filled above
                hw = std::make_shared<gd::HostWorld>();
                gd::build_host_world(*sit->second, params, A, del, ndel, *hw);
                // the row kernel's 32-byte road record restores the z scale from the entity type (1 for stop signs, 0.1
                // for everything else: scene.cpp put_road callers); checked here, before anything of this call is uploaded
                for (size_t r = 0; r * 8 < hw->road_aux.size(); r++) {
                    const float *a = &hw->road_aux[r * 8];
                    if (a[4] != (static_cast<int>(a[5]) == gd::ET_StopSign ? 1.f : 0.1f))
                        throw std::runtime_error("road record: unexpected z scale for this entity type");
                }
                world_cache.emplace(key, hw);
            }
            st.traj.insert(st.traj.end(), hw->trajectory.begin(), hw->trajectory.end());
            // map_observation_tensor rows + MapObservation::zero() padding (src/level_gen.cpp:331-335)
            const size_t m0 = st.map_obs.size();
            st.map_obs.resize(m0 + static_cast<size_t>(GD_MAX_ROAD_ENTITIES) * 9, 0.f);
            std::memcpy(st.map_obs.data() + m0, hw->map_obs.data(), sizeof(float) * hw->map_obs.size());
            for (int r = hw->num_roads; r < GD_MAX_ROAD_ENTITIES; r++) {
                st.map_obs[m0 + static_cast<size_t>(r) * 9 + 7] = -1.f;
                st.map_obs[m0 + static_cast<size_t>(r) * 9 + 8] = -1.f;
            }
            for (int a = 0; a < A; a++) {  // AoS rows -> SoA planes
                st.planes[0].push_back(hw->size[a * 3 + 0]);
                st.planes[1].push_back(hw->size[a * 3 + 1]);
                st.planes[2].push_back(hw->size[a * 3 + 2]);
                st.planes[3].push_back(hw->scale[a * 2 + 0]);
                st.planes[4].push_back(hw->scale[a * 2 + 1]);
                st.planes[5].push_back(hw->goal[a * 2 + 0]);
                st.planes[6].push_back(hw->goal[a * 2 + 1]);
            }
            st.etype.insert(st.etype.end(), hw->etype.begin(), hw->etype.end());
            st.agent_id.insert(st.agent_id.end(), hw->agent_id.begin(), hw->agent_id.end());
            st.resp.insert(st.resp.end(), hw->resp.begin(), hw->resp.end());
            st.controlled.insert(st.controlled.end(), hw->controlled.begin(), hw->controlled.end());
            st.metadata.insert(st.metadata.end(), hw->metadata.begin(), hw->metadata.end());
            st.deleted.insert(st.deleted.end(), del, del + A);
            st.means.insert(st.means.end(), hw->mean, hw->mean + 3);
            st.map_name.insert(st.map_name.end(), hw->map_name, hw->map_name + 32);
            st.scenario_id.insert(st.scenario_id.end(), hw->scenario_id, hw->scenario_id + 32);
            st.shape.push_back(hw->num_agents);
            st.shape.push_back(hw->num_roads);
            WorldHost &host = world_host[w];
            host.xy = hw->road_xy;
            host.agents = hw->num_agents;
            host.resp = hw->resp;
            host.aux = hw->road_aux;
            host.boxes = hw->boxes;
            host.grid = gd::GridHdr{hw->grid_ox, hw->grid_oy, 1.f / hw->grid_cell, hw->grid_nx, hw->grid_ny, 0, 0, 0};
            host.cell_off = hw->cell_off;
            host.cell_items = hw->cell_items;
            build_road_grid(host);
            rebuilt[w] = 1;
        }
        flush(run_start, run_len);
        // repack the road CSR
        std::vector<WorldHost> &wh = world_host;
        std::vector<int32_t> road_off(W + 1, 0), box_off(W + 1, 0);
        for (int w = 0; w < W; w++) {
            road_off[w + 1] = road_off[w] + static_cast<int32_t>(wh[w].xy.size() / 2);
            box_off[w + 1] = box_off[w] + static_cast<int32_t>(wh[w].boxes.size());
        }
        const size_t nroad = road_off[W], nbox = box_off[W];
        if (road_xy.fit(nroad, d.road_xy)) HIP_CHECK(hipMemset(road_xy.mem.get(), 0, road_xy.mem.bytes()));
        if (road_aux.fit(nroad, d.road_aux)) HIP_CHECK(hipMemset(road_aux.mem.get(), 0, road_aux.mem.bytes()));
        if (road_rec.fit(nroad, d.road_rec)) HIP_CHECK(hipMemset(road_rec.mem.get(), 0, road_rec.mem.bytes()));
        boxes.fit(nbox, d.boxes);
        {
            std::vector<float> xy(nroad * 2), aux(nroad * 8);
            std::vector<gd::RoadBox> bx(nbox);
            for (int w = 0; w < W; w++) {
                std::copy(wh[w].xy.begin(), wh[w].xy.end(), xy.begin() + static_cast<size_t>(road_off[w]) * 2);
                std::copy(wh[w].aux.begin(), wh[w].aux.end(), aux.begin() + static_cast<size_t>(road_off[w]) * 8);
                std::copy(wh[w].boxes.begin(), wh[w].boxes.end(), bx.begin() + box_off[w]);
            }
            if (nroad) {
                road_xy.upload(xy.data(), nroad);
                road_aux.upload(aux.data(), nroad);
                // the row kernel's 32-byte record: aux is (qw, qz, d0, d1, d2, type, id, mapType); d2 is a function of the
                // type (validated while staging), which the kernel restores
                std::vector<float> rec(nroad * 8);
                for (size_t r = 0; r < nroad; r++) {
                    const float *a = &aux[r * 8];
                    const uint32_t bits = (static_cast<uint32_t>(static_cast<int>(a[5])) & 0xffu) |
                                          (static_cast<uint32_t>(static_cast<int>(a[7]) + 1) << 8);
                    float fb;
                    std::memcpy(&fb, &bits, sizeof(fb));
                    const float row[8] = {xy[r * 2], xy[r * 2 + 1], a[0], a[1], a[2], a[3], a[6], fb};
                    std::copy(row, row + 8, rec.begin() + r * 8);
                }
                road_rec.upload(rec.data(), nroad);
            }
            HIP_CHECK(hipMemsetAsync(d.sel_hdr, 0xff, sizeof(float4) * 2 * static_cast<size_t>(W) * d.A, stream));  // count -1: nothing selected yet (ordered before the kernels of this stream)
            boxes.upload(bx.data(), nbox);
        }
        {
            size_t ncell = 0, nitem = 0;
            std::vector<gd::GridHdr> hdr(W);
            for (int w = 0; w < W; w++) {
                wh[w].grid.cell_base = static_cast<int>(ncell);
                wh[w].grid.item_base = static_cast<int>(nitem);
                hdr[w] = wh[w].grid;
                ncell += wh[w].cell_off.size();
                nitem += wh[w].cell_items.size();
            }
            cell_off.fit(ncell, d.cell_off);
            cell_items.fit(nitem, d.cell_items);
            cell_hdr.fit(nitem, d.cell_hdr);
            std::vector<int32_t> co(ncell), ci(nitem);
            for (int w = 0; w < W; w++) {
                std::copy(wh[w].cell_off.begin(), wh[w].cell_off.end(), co.begin() + hdr[w].cell_base);
                std::copy(wh[w].cell_items.begin(), wh[w].cell_items.end(), ci.begin() + hdr[w].item_base);
            }
            cell_off.upload(co.data(), ncell);
            cell_items.upload(ci.data(), nitem);
            {
                std::vector<float> ch(nitem * 4);
                for (int w = 0; w < W; w++) {
                    const std::vector<int32_t> &items = wh[w].cell_items;
                    for (size_t i = 0; i < items.size(); i++) {
                        const gd::RoadBox &b = wh[w].boxes[items[i]];
                        float *o = &ch[(static_cast<size_t>(hdr[w].item_base) + i) * 4];
                        // (centre, bounding radius, entity type | local box index << 8): what the cull needs and where the box is
                        const uint32_t packed = (static_cast<uint32_t>(static_cast<int>(b.type)) & 0xffu) | (static_cast<uint32_t>(items[i]) << 8);
                        o[0] = b.cx; o[1] = b.cy; o[2] = b.radius;
                        std::memcpy(&o[3], &packed, sizeof(packed));
                    }
                }
                cell_hdr.upload(ch.data(), nitem);
            }
            HIP_CHECK(hipMemcpy(d_grid, hdr.data(), sizeof(gd::GridHdr) * W, hipMemcpyHostToDevice));
        }
        HIP_CHECK(hipMemcpy(d_road_off, road_off.data(), sizeof(int32_t) * (W + 1), hipMemcpyHostToDevice));
        upload_road_grids();
        {
            // longest-first launch order of the road kernel: its time per world grows with the road count (the kernel
            // re-sorts by measured cycles after every launch; this is the order of the first one)
            const int parts = d.A / GD_MAP_OBS_AW;
            std::vector<int32_t> order(W);
            for (int w = 0; w < W; w++) order[w] = w;
            std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
                return road_off[x + 1] - road_off[x] > road_off[y + 1] - road_off[y];
            });
            std::vector<int32_t> waves(static_cast<size_t>(W) * parts);
            for (int k = 0; k < W; k++)
                for (int q = 0; q < parts; q++) waves[static_cast<size_t>(k) * parts + q] = order[k] * parts + q;
            HIP_CHECK(hipMemcpy(d.wave_order, waves.data(), sizeof(int32_t) * waves.size(), hipMemcpyHostToDevice));
            HIP_CHECK(hipMemsetAsync(d.wave_cost, 0, sizeof(uint32_t) * waves.size(), stream));
        }
        HIP_CHECK(hipMemcpy(d_box_off, box_off.data(), sizeof(int32_t) * (W + 1), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d.rebuilt_flags, rebuilt.data(), sizeof(int32_t) * W, hipMemcpyHostToDevice));
        choose_set_schedule();
        {
            // the box around every world's roads: an agent farther than the radius from it has no road in reach (linear scan,
            // rank replay)
            std::vector<float> bb(static_cast<size_t>(W) * 4);
            for (int w = 0; w < W; w++) {
                float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
                const std::vector<float> &xy = wh[w].xy;
                for (size_t r = 0; r * 2 < xy.size(); r++) {
                    lo_x = std::min(lo_x, xy[2 * r]); hi_x = std::max(hi_x, xy[2 * r]);
                    lo_y = std::min(lo_y, xy[2 * r + 1]); hi_y = std::max(hi_y, xy[2 * r + 1]);
                }
                bb[w * 4 + 0] = lo_x; bb[w * 4 + 1] = lo_y; bb[w * 4 + 2] = hi_x; bb[w * 4 + 3] = hi_y;
            }
            HIP_CHECK(hipMemcpy(d_road_bbox, bb.data(), bb.size() * sizeof(float), hipMemcpyHostToDevice));
            std::vector<float> rbmax(W, 0.f);  // (road_aux: qw qz d0 d1 | d2 type id mapType)
            for (int w = 0; w < W; w++) {
                const std::vector<float> &aux = wh[w].aux;
                for (size_t r = 0; r * 8 < aux.size(); r++)
                    rbmax[w] = std::max(rbmax[w], std::sqrt(aux[r * 8 + 2] * aux[r * 8 + 2] + aux[r * 8 + 3] * aux[r * 8 + 3]));
            }
            HIP_CHECK(hipMemcpy(d_road_rbmax, rbmax.data(), rbmax.size() * sizeof(float), hipMemcpyHostToDevice));
            // the circle around every GD_LIN_BLK consecutive road points of a world (centre of their bounding box, the largest
            // distance from it to one of them, rounded up)
            std::vector<int32_t> boff(W + 1, 0);
            for (int w = 0; w < W; w++) boff[w + 1] = boff[w] + static_cast<int32_t>((wh[w].xy.size() / 2 + GD_LIN_BLK - 1) / GD_LIN_BLK);
            std::vector<float> blk(static_cast<size_t>(boff[W]) * 4 + 4, 0.f);
            for (int w = 0; w < W; w++) {
                const std::vector<float> &xy = wh[w].xy;
                const size_t nr = xy.size() / 2;
                for (size_t b = 0; b * GD_LIN_BLK < nr; b++) {
                    const size_t r_lo = b * GD_LIN_BLK, r_hi = std::min(nr, r_lo + GD_LIN_BLK);
                    float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
                    for (size_t r = r_lo; r < r_hi; r++) {
                        lo_x = std::min(lo_x, xy[2 * r]); hi_x = std::max(hi_x, xy[2 * r]);
                        lo_y = std::min(lo_y, xy[2 * r + 1]); hi_y = std::max(hi_y, xy[2 * r + 1]);
                    }
                    const float cx = 0.5f * (lo_x + hi_x), cy = 0.5f * (lo_y + hi_y);
                    float rad = 0.f;
                    for (size_t r = r_lo; r < r_hi; r++)
                        rad = std::max(rad, std::sqrt((xy[2 * r] - cx) * (xy[2 * r] - cx) + (xy[2 * r + 1] - cy) * (xy[2 * r + 1] - cy)));
                    float *o = &blk[(static_cast<size_t>(boff[w]) + b) * 4];
                    o[0] = cx; o[1] = cy; o[2] = rad * 1.0001f + 1e-3f; o[3] = 0.f;
                }
            }
            road_blk.fit(blk.size() / 4, d.road_blk);  // (never empty: one spare circle behind the last world's)
            road_blk.upload(blk.data(), blk.size() / 4);
            HIP_CHECK(hipMemcpy(d_blk_off, boff.data(), sizeof(int32_t) * (W + 1), hipMemcpyHostToDevice));
            // no row written before this call describes the worlds as they are now (roads, agent slots): every pose stamp dies
            HIP_CHECK(hipMemsetAsync(d.pose_stamp, 0xff, sizeof(uint4) * static_cast<size_t>(W) * A, stream));
            HIP_CHECK(hipMemsetAsync(d.bev_dirty, 1, sizeof(int32_t) * static_cast<size_t>(W) * A, stream));
            HIP_CHECK(hipMemsetAsync(d.lidar_dirty, 1, sizeof(int32_t) * static_cast<size_t>(W) * A, stream));
            HIP_CHECK(hipMemsetAsync(d.lidar_head, 0xff, sizeof(float) * static_cast<size_t>(W) * A, stream));
        }
        if (rk_possible) {
            // Which worlds take the rank replay (neither path changes a result).  Measured at 64 agent slots (road
            // observation, ms): 1024 worlds x 4096 roads 1.19 ranked / 1.84 on keys; 1024 Waymo tiles (346-873 roads) 0.44 /
            // 0.47; 4096 Waymo tiles 0.94 / 1.74.  The rank kernels' fixed costs (seven launches, a replay as long as the
            // longest agent's candidate list) pay once k_map_obs's workgroups fill the chip: large worlds always, every
            // world with at least K roads from one full generation of k_map_obs workgroups on.  GPUDRIVE_RANK_MIN_ROADS
            // pins the threshold.
            int groups = 0;
            for (int w = 0; w < W; w++) groups += (wh[w].agents + 31) / 32;
            const char *pin = std::getenv("GPUDRIVE_RANK_MIN_ROADS");
            d.rk_min_roads = pin ? std::atoi(pin) : (groups >= 4 * cu_count ? GD_MAP_OBS_K : 1536);
            // Worlds of every size take it since round 4 (agents whose candidates overflow the standard ranking's 1272 go to the
            // long-list instantiation, 2552; groups that keep overflowing even that bypass the rank kernels on their own:
            // rk_streak).  GPUDRIVE_RANK_MAX_ROADS pins an upper limit for experiments.
            const char *pin_max = std::getenv("GPUDRIVE_RANK_MAX_ROADS");
            d.rk_max_roads = pin_max ? std::atoi(pin_max) : GD_MAX_ROAD_ENTITIES;
            d.rk_on = 0;
            for (int w = 0; w < W; w++) {
                const int R = road_off[w + 1] - road_off[w];
                if (R >= std::max(d.rk_min_roads, GD_MAP_OBS_K) && R <= d.rk_max_roads) d.rk_on = 1;
            }
            if (d.rk_on && ensure_rank_buffers()) reset_rank_state();
        }
        {
            // one BEV workgroup per LIVE agent: a workgroup that only finds out it has no agent still has to be given
            // its 48 KB of LDS and eight waves first
            std::vector<int32_t> live;
            live.reserve(static_cast<size_t>(W) * A);
            for (int a = 0; a < A; a++)  // agent-major: consecutive workgroups belong to different worlds
                for (int w = 0; w < W; w++)
                    if (a < wh[w].agents) live.push_back(w * A + a);
            d.live_count = static_cast<int>(live.size());
            if (!live.empty()) HIP_CHECK(hipMemcpy(d.live_list, live.data(), sizeof(int32_t) * live.size(), hipMemcpyHostToDevice));
            // likewise the set-order road kernel's workgroups (4 waves x set_apw agents each)
            std::vector<int32_t> groups;
            const int per = 4 * d.set_apw;
            for (int g = 0; g * per < A; g++)  // group-major: consecutive workgroups belong to different worlds
                for (int w = 0; w < W; w++)
                    if (g * per < wh[w].agents) groups.push_back(w << 8 | g);
            d.set_group_count = static_cast<int>(groups.size());
            if (!groups.empty()) HIP_CHECK(hipMemcpy(d.set_groups, groups.data(), sizeof(int32_t) * groups.size(), hipMemcpyHostToDevice));
        }
        {
            // The linear scan's work lists: the live agents as (world << 8 | agent), world-major inside eight classes, the classes
            // interleaved workgroup by workgroup (4 * lin_apw entries each): workgroup b runs on XCD b % 8 (MI355X_MICROARCH.md,
            // dispatch), so every workgroup that holds agents of a world -- and the world's road arrays -- stays on one XCD's L2.
            // Classes are filled greedily (fewest entries so far) so that ragged batches leave few filler entries.  Two lists:
            // every live agent (reset passes), and the agents that can move (step passes).  A `Static` agent's rows were written
            // by the reset pass that follows every rebuild, and its own movement never moves it -- but under AgentRemoved a
            // Static agent that is hit is moved to the padding position by the next step (reference src/sim.cpp:302-313, the
            // collision switch comes before the Static early return), so there the step passes take every live agent too
            // (the pose stamps still skip the ones that did not move).
            const int per = 4 * d.lin_apw;
            auto build = [&](bool dyn_only, std::vector<int32_t> &list) -> int {
                std::vector<int32_t> seq[8];
                for (int w = 0; w < W; w++) {
                    std::vector<int32_t> mine;
                    for (int a = 0; a < wh[w].agents; a++)
                        if (!dyn_only || wh[w].resp[a] != gd::RESP_Static) mine.push_back(w << 8 | a);
                    if (mine.empty()) continue;
                    int c = w % 8;
                    for (int k = 0; k < 8; k++)
                        if (seq[k].size() + 4 * static_cast<size_t>(A) < seq[c].size()) c = k;  // only when a class runs far ahead
                    seq[c].insert(seq[c].end(), mine.begin(), mine.end());
                }
                size_t blocks = 0;
                for (auto &q : seq) blocks = std::max(blocks, (q.size() + per - 1) / per);
                list.assign(blocks * 8 * per, -1);
                for (int c = 0; c < 8; c++)
                    for (size_t j = 0; j < seq[c].size(); j++) list[((j / per) * 8 + c) * per + j % per] = seq[c][j];
                return static_cast<int>(blocks * 8);
            };
            std::vector<int32_t> full, dyn;
            d.lin_blocks = build(false, full);
            d.lin_blocks_dyn = build(params.collisionBehaviour != GD_COLLISION_AGENT_REMOVED, dyn);
            lin_static_agents = 0;
            for (int32_t e : full) lin_static_agents += e >= 0;
            for (int32_t e : dyn) lin_static_agents -= e >= 0;
            if (full.size() > lin_cap || dyn.size() > lin_cap) throw std::runtime_error("linear-scan work list: more entries than the list holds");
            if (!full.empty()) HIP_CHECK(hipMemcpy(d_lin_list, full.data(), sizeof(int32_t) * full.size(), hipMemcpyHostToDevice));
            if (!dyn.empty()) HIP_CHECK(hipMemcpy(d_lin_list_dyn, dyn.data(), sizeof(int32_t) * dyn.size(), hipMemcpyHostToDevice));
            d.lin_list = d_lin_list;
            d.lin_list_dyn = d_lin_list_dyn;
        }
        launch(gd::KERNEL_PADDING, false);
        // the packed observation's rows of padding agents come from the raw padding rows just written (the live agents' rows are
        // written by the reset pass that follows every rebuild)
        if (d.pack && d.pack_rows) gd::launch_pack_obs_rows(d, stream, d.pack, d.pack_weights);
        else if (d.pack) gd::launch_pack_obs(d, stream, d.pack);
    }

    // detach the packed buffer (either kind): the raw tensors are written again from the next pass on; bring them up to date now
    void detach_packed() {
        HIP_CHECK(hipStreamSynchronize(stream));
        drop_graph();
        d.pack = nullptr;
        d.pack_only = 0;
        d.pack_rows = 0;
        d.pack_weights = nullptr;
        HIP_CHECK(hipMemsetAsync(d.pose_stamp, 0xff, sizeof(uint4) * static_cast<size_t>(W) * A, stream));
        reset_flagged(false);
    }

    // attach `out` as the packed buffer: everything once from the raw tensors (the padding agents' rows never change between
    // rebuilds); then every pass of the step kernels writes the live agents' rows in place.  Every pose stamp dies: the next
    // pass writes every live agent's road columns, whatever was skipped before.  rows: out is [n_rows][D] (learner rows);
    // weights (with rows): out is [n_rows][D + 3], the conditioned rows with the slots' reward weights.
    void attach_packed(float *out, bool only, bool rows, const float *weights = nullptr) {
        HIP_CHECK(hipStreamSynchronize(stream));
        drop_graph();
        d.pack = nullptr;
        d.pack_only = 0;
        d.pack_rows = 0;
        d.pack_weights = nullptr;
        HIP_CHECK(hipMemsetAsync(d.pose_stamp, 0xff, sizeof(uint4) * static_cast<size_t>(W) * A, stream));
        reset_flagged(false);  // raw tensors up to date (a previous pack_only attachment left them stale)
        if (rows) gd::launch_pack_obs_rows(d, stream, out, weights);
        else gd::launch_pack_obs(d, stream, out);
        HIP_CHECK(hipGetLastError());
        d.pack = out;
        d.pack_only = only ? 1 : 0;
        d.pack_rows = rows ? 1 : 0;
        d.pack_weights = rows ? weights : nullptr;
    }

    // the packed observation can be written where the rows are produced by every road path -- the linear scan, set order
    // (fused write-out), and k_map_rows behind the reference-order selections and the unfused set-order one -- except the
    // linear scan's legacy path (GPUDRIVE_LINEAR_LEGACY=1, an A/B switch)
    bool direct_pack_supported() const {
        if (params.disableClassicalObs) return false;
        if (params.roadObservationAlgorithm != GD_ROADS_K_NEAREST) return d.lin_on != 0;
        return true;
    }

    // Uniform grid over the (x, y) of ALL roads of world w: cells of at least 16 m, at most 64 x 64 of them; a road
    // belongs to the cell its point falls into, and a cell lists its roads in ascending index.
    static void build_road_grid(WorldHost &world) {
        const std::vector<float> &xy = world.xy;
        const size_t n = xy.size() / 2;
        gd::GridHdr g{0.f, 0.f, 1.f, 1, 1, 0, 0, 0};
        std::vector<int32_t> off(2, 0);
        std::vector<uint16_t> items(n);
        if (n) {
            float minx = xy[0], maxx = xy[0], miny = xy[1], maxy = xy[1];
            for (size_t r = 1; r < n; r++) {
                minx = std::min(minx, xy[2 * r]); maxx = std::max(maxx, xy[2 * r]);
                miny = std::min(miny, xy[2 * r + 1]); maxy = std::max(maxy, xy[2 * r + 1]);
            }
            const float cell = std::max(GD_GRID_MIN_CELL, std::max(maxx - minx, maxy - miny) / 64.f + 1e-3f);
            g.ox = minx; g.oy = miny; g.inv_cell = 1.f / cell;
            g.nx = std::max(1, std::min(64, static_cast<int>((maxx - minx) * g.inv_cell) + 1));
            g.ny = std::max(1, std::min(64, static_cast<int>((maxy - miny) * g.inv_cell) + 1));
            const int nc = g.nx * g.ny;
            std::vector<int32_t> cell_of(n);
            off.assign(nc + 1, 0);
            for (size_t r = 0; r < n; r++) {
                const int cx = std::max(0, std::min(g.nx - 1, static_cast<int>((xy[2 * r] - g.ox) * g.inv_cell)));
                const int cy = std::max(0, std::min(g.ny - 1, static_cast<int>((xy[2 * r + 1] - g.oy) * g.inv_cell)));
                cell_of[r] = cy * g.nx + cx;
                off[cell_of[r] + 1]++;
            }
            for (int c = 0; c < nc; c++) off[c + 1] += off[c];
            std::vector<int32_t> fill(off.begin(), off.end() - 1);
            for (size_t r = 0; r < n; r++) items[fill[cell_of[r]]++] = static_cast<uint16_t>(r);  // ascending r within a cell
        }
        world.rgrid = g;
        world.rcell_off = std::move(off);
        world.rcell_items = std::move(items);
    }

    void upload_road_grids() {
        size_t ncell = 0, nitem = 0;
        std::vector<gd::GridHdr> hdr(W);
        for (int w = 0; w < W; w++) {
            world_host[w].rgrid.cell_base = static_cast<int>(ncell);
            world_host[w].rgrid.item_base = static_cast<int>(nitem);
            hdr[w] = world_host[w].rgrid;
            ncell += world_host[w].rcell_off.size();
            nitem += world_host[w].rcell_items.size();
        }
        rcell_off.fit(ncell, d.rcell_off);
        rcell_items.fit(nitem, d.rcell_items);
        rcell_xy.fit(nitem, d.rcell_xy);
        rcell_pos.fit(nitem, d.rcell_pos);
        std::vector<int32_t> co(ncell);
        std::vector<uint16_t> ci(nitem);
        std::vector<float> cxy(nitem * 2);
        std::vector<uint16_t> cpos(nitem);  // (a world's items are its roads, one each: item_base is also its first road)
        for (int w = 0; w < W; w++) {
            const WorldHost &x = world_host[w];
            std::copy(x.rcell_off.begin(), x.rcell_off.end(), co.begin() + hdr[w].cell_base);
            std::copy(x.rcell_items.begin(), x.rcell_items.end(), ci.begin() + hdr[w].item_base);
            for (size_t k = 0; k < x.rcell_items.size(); k++) {
                const size_t r = x.rcell_items[k], o = (static_cast<size_t>(hdr[w].item_base) + k) * 2;
                cxy[o] = x.xy[2 * r];
                cxy[o + 1] = x.xy[2 * r + 1];
                cpos[static_cast<size_t>(hdr[w].item_base) + r] = static_cast<uint16_t>(k);
            }
        }
        rcell_off.upload(co.data(), ncell);
        rcell_items.upload(ci.data(), nitem);
        rcell_xy.upload(cxy.data(), nitem);
        rcell_pos.upload(cpos.data(), nitem);
        HIP_CHECK(hipMemcpy(d_rgrid, hdr.data(), sizeof(gd::GridHdr) * W, hipMemcpyHostToDevice));
        // the roads changed: no previous selection bounds the next one
        std::vector<float> prev(static_cast<size_t>(W) * A * 4, 0.f);
        for (size_t i = 0; i < static_cast<size_t>(W) * A; i++) prev[i * 4 + 2] = INFINITY;
        HIP_CHECK(hipMemcpy(d.knn_prev, prev.data(), prev.size() * sizeof(float), hipMemcpyHostToDevice));
    }

    // No checkpoint of a previous selection survives a change of the worlds' roads or agent slots: in its next selection
    // every agent is bounded afresh inside k_knn_scan (a distance histogram at geometric road counts, map_obs_rank.hip).
    void reset_rank_state() {
        HIP_CHECK(hipMemset(d.cp_hdr, 0, sizeof(float4) * 2 * static_cast<size_t>(W) * A));
        HIP_CHECK(hipMemset(d.rk_fallback, 0, sizeof(int32_t) * (static_cast<size_t>(W) * A / 32)));
        HIP_CHECK(hipMemset(d.rk_streak, 0, sizeof(int32_t) * (static_cast<size_t>(W) * A / 32)));
        HIP_CHECK(hipMemset(d.rk_hist, 0, sizeof(int32_t) * GD_RANK_AUDIT));  // bin counts, the lists of ranked agents: empty (the audit counter behind them keeps counting)
        HIP_CHECK(hipMemset(d.rk_hist + GD_RH_LONG, 0, sizeof(int32_t) * (GD_RH_SIZE - GD_RH_LONG)));  // the long list: empty; k_knn_rank's cursors: at the lists' heads
    }

    void do_reset(const std::vector<int32_t> &flags) {
        upload_flags(d.reset_flags, flags);
        reset_flagged(false);
    }

    // resetSystem + the observation half of the task graph (src/sim.cpp:150-166, 960-971) for the worlds
    // whose reset flag is set ON THE DEVICE (by the upload above or by k_episode_step).  Like the
    // reference's Reset graph the observation systems re-run for EVERY world (not idempotent in the
    // reference: the collision system sees the already decremented step counter, so a reset anywhere can
    // raise collision flags elsewhere -- reproduced, and tested).  `gated`: the host does not know whether
    // k_episode_step flagged anything; the kernels are launched regardless and return at once unless
    // *any_reset is set, so a step without finished worlds costs three empty launches and no host sync.
    void reset_flagged(bool gated) {
        d.gate_any = gated ? 1 : 0;
        if (!gated) full_pass_next = false;  // (an ungated reset pass visits every live agent: nothing is owed any more)
        try {
            launch(gd::KERNEL_RESET, false);
            run_rest(false);
        } catch (...) {
            d.gate_any = 0;
            throw;
        }
        d.gate_any = 0;
    }
};

namespace {

template <typename F>
int guarded(F &&f) {
    try {
        f();
        return GD_OK;
    } catch (const HipError &e) {
        return fail(GD_ERR_DEVICE, e.what());
    } catch (const std::invalid_argument &e) {
        const std::string m = e.what();
        return fail(m.find("cannot open") != std::string::npos ? GD_ERR_IO : GD_ERR_INVALID, m);
    } catch (const std::exception &e) {
        return fail(GD_ERR_PARSE, e.what());
    }
}

}  // namespace

extern "C" {

const char *gd_version(void) { return "gpudrive_amd 0.1 (gfx950)"; }
const char *gd_last_error(void) { return g_last_error.c_str(); }

void gd_default_params(gd_params *p) {  // src/init.hpp:111-127
    std::memset(p, 0, sizeof(*p));
    p->collisionBehaviour = GD_COLLISION_AGENT_STOP;
    p->maxNumControlledAgents = 10000;
    p->IgnoreNonVehicles = 0;
    p->roadObservationAlgorithm = GD_ROADS_K_NEAREST;
    p->initOnlyValidAgentsAtFirstStep = 1;
    p->isStaticAgentControlled = 0;
    p->dynamicsModel = GD_DYNAMICS_CLASSIC;
}

int gd_tensor_shape(int32_t id, int32_t W, int32_t A, gd_tensor_desc *out) {
    if (!out || id < 0 || id >= GD_T_COUNT || W < 1 || A < 2) return fail(GD_ERR_INVALID, "gd_tensor_shape: bad argument");
    const TensorSpec s = tensor_spec(id, W, A);
    out->data = nullptr;
    out->dtype = s.dtype;
    out->ndim = s.ndim;
    for (int i = 0; i < 5; i++) out->dims[i] = i < s.ndim ? s.dims[i] : 1;
    out->nbytes = spec_bytes(s);
    return GD_OK;
}

int gd_create(const gd_config *cfg, const gd_params *params, const char *const *scenes, gd_sim **out) {
    if (!cfg || !params || !scenes || !out) return fail(GD_ERR_INVALID, "gd_create: null argument");
    if (cfg->num_worlds < 1) return fail(GD_ERR_INVALID, "gd_create: num_worlds must be >= 1");
    if (cfg->max_agents != 64 && cfg->max_agents != 128)
        return fail(GD_ERR_INVALID, "gd_create: max_agents must be 64 or 128");
    if (params->rewardType == GD_REWARD_DENSE)
        return fail(GD_ERR_UNSUPPORTED, "RewardType::Dense is assert(false) in the reference (src/sim.cpp:579-583)");
    *out = nullptr;
    std::unique_ptr<gd_sim> s(new gd_sim());
    const int rc = guarded([&]() {
        int ndev = 0;
        HIP_CHECK(hipGetDeviceCount(&ndev));
        if (ndev < 1) throw HipError("no HIP device visible: the HIP path is mandatory, there is no CPU fallback");
        HIP_CHECK(hipSetDevice(cfg->device_id));
        s->cfg = *cfg;
        s->params = *params;
        s->W = cfg->num_worlds;
        s->A = cfg->max_agents;
        s->stream = static_cast<hipStream_t>(cfg->stream);
        const int W = s->W, A = s->A;
        for (int w = 0; w < W; w++) {
            if (!scenes[w]) throw std::invalid_argument("gd_create: null scene path");
            s->scenes.emplace_back(scenes[w]);
        }
        s->deleted.assign(static_cast<size_t>(W) * A, -1);  // src/sim.cpp:1003-1006
        s->world_host.resize(W);
        for (int id = 0; id < GD_T_COUNT; id++) {
            if (id == GD_T_BEV && !cfg->alloc_bev && !cfg->external[id]) continue;
            const int64_t bytes = spec_bytes(tensor_spec(id, W, A));
            if (!cfg->external[id]) s->exported_mem[id] = gd::DevMem(bytes);
            s->exported[id] = cfg->external[id] ? cfg->external[id] : s->exported_mem[id].get();
            HIP_CHECK(hipMemset(s->exported[id], 0, bytes));
        }
        gd::DevSim &d = s->d;
        d.W = W;
        d.A = A;
        d.p = *params;
        d.knn_order = cfg->knn_order;
        // (not on the legacy null stream: it synchronises with every blocking stream and cannot be captured)
        d.split_partner = (s->stream != nullptr && std::getenv("GPUDRIVE_SPLIT_PARTNER") != nullptr) ? 1 : 0;
        hipStream_t side = nullptr;
        HIP_CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        s->side.reset(side);
        s->ev_fork = make_event(hipEventDisableTiming);
        s->ev_join = make_event(hipEventDisableTiming);
        d.step_dbg = 0;
#ifdef GD_DIAG
        if (const char *e = std::getenv("GPUDRIVE_STEP_DBG")) d.step_dbg = std::atoi(e);
#endif
        {
            (void)hipDeviceGetAttribute(&s->cu_count, hipDeviceAttributeMultiprocessorCount, cfg->device_id);
            d.set_fused_rows = 0;  // chosen with the worlds (rebuild_worlds -> choose_set_schedule)
            d.set_apw = 16;
        }
        d.lidar_half_angle = cfg->lidar_half_angle;
        {
            // radiusFilter keeps length() <= radius (src/knn.hpp:88); on squared keys: key <= kmax
            const float r = params->observationRadius;
            float k = r * r;
            while (k > 0.f && sqrtf(k) > r) k = std::nextafterf(k, 0.f);
            while (sqrtf(std::nextafterf(k, INFINITY)) <= r) k = std::nextafterf(k, INFINITY);
            d.radius_key_max = r >= 0.f ? k : -1.f;
        }
        d.action = static_cast<float *>(s->exported[GD_T_ACTION]);
        d.reward = static_cast<float *>(s->exported[GD_T_REWARD]);
        d.done = static_cast<int32_t *>(s->exported[GD_T_DONE]);
        d.info = static_cast<int32_t *>(s->exported[GD_T_INFO]);
        d.self_obs = static_cast<float *>(s->exported[GD_T_SELF_OBS]);
        d.abs_obs = static_cast<float *>(s->exported[GD_T_ABS_OBS]);
        d.partner = static_cast<float *>(s->exported[GD_T_PARTNER_OBS]);
        d.agent_map = static_cast<float *>(s->exported[GD_T_AGENT_MAP_OBS]);
        d.map_obs = static_cast<float *>(s->exported[GD_T_MAP_OBS]);
        d.lidar = static_cast<float *>(s->exported[GD_T_LIDAR]);
        d.bev = static_cast<float *>(s->exported[GD_T_BEV]);
        d.steps = static_cast<uint32_t *>(s->exported[GD_T_STEPS_REMAINING]);
        d.shape = static_cast<int32_t *>(s->exported[GD_T_SHAPE]);
        d.controlled = static_cast<int32_t *>(s->exported[GD_T_CONTROLLED_STATE]);
        d.resp_export = static_cast<int32_t *>(s->exported[GD_T_RESPONSE_TYPE]);
        d.traj = static_cast<float *>(s->exported[GD_T_EXPERT_TRAJECTORY]);
        d.means = static_cast<float *>(s->exported[GD_T_WORLD_MEANS]);
        d.metadata = static_cast<int32_t *>(s->exported[GD_T_METADATA]);
        d.deleted = static_cast<int32_t *>(s->exported[GD_T_DELETED_AGENTS]);
        d.map_name = static_cast<int32_t *>(s->exported[GD_T_MAP_NAME]);
        d.scenario_id = static_cast<int32_t *>(s->exported[GD_T_SCENARIO_ID]);
        const size_t WA = static_cast<size_t>(W) * A;
        d.px = s->alloc_internal<float>(WA); d.py = s->alloc_internal<float>(WA); d.pz = s->alloc_internal<float>(WA);
        d.qw = s->alloc_internal<float>(WA); d.qz = s->alloc_internal<float>(WA);
        d.vx = s->alloc_internal<float>(WA); d.vy = s->alloc_internal<float>(WA); d.vz = s->alloc_internal<float>(WA);
        d.collided = s->alloc_internal<int32_t>(WA);
        d.len = s->alloc_internal<float>(WA); d.wid = s->alloc_internal<float>(WA); d.hgt = s->alloc_internal<float>(WA);
        d.sc0 = s->alloc_internal<float>(WA); d.sc1 = s->alloc_internal<float>(WA);
        d.goal_x = s->alloc_internal<float>(WA); d.goal_y = s->alloc_internal<float>(WA);
        d.etype = s->alloc_internal<int32_t>(WA); d.agent_id = s->alloc_internal<int32_t>(WA);
        d.resp = s->alloc_internal<int32_t>(WA);
        d.sel_idx = s->alloc_internal<uint16_t>(static_cast<size_t>(WA) * GD_MAP_OBS_K);
        d.sel_hdr = s->alloc_internal<float4>(static_cast<size_t>(WA) * 2);
        d.sel_slot = s->alloc_internal<uint8_t>(static_cast<size_t>(WA) * GD_MAP_OBS_K);
        d.reset_flags = s->alloc_internal<int32_t>(W);
        d.rebuilt_flags = s->alloc_internal<int32_t>(W);
        d.any_reset = s->alloc_internal<int32_t>(1);
        d.gate_any = 0;
        d.road_off = s->d_road_off = s->alloc_internal<int32_t>(W + 1);
        d.live_list = s->alloc_internal<int32_t>(WA);
        d.live_count = 0;
        d.set_groups = s->alloc_internal<int32_t>(WA);
        d.set_group_count = 0;
        d.wave_order = s->alloc_internal<int32_t>(static_cast<size_t>(W) * (A / GD_MAP_OBS_AW));
        d.wave_cost = s->alloc_internal<uint32_t>(static_cast<size_t>(W) * (A / GD_MAP_OBS_AW));
        d.box_off = s->d_box_off = s->alloc_internal<int32_t>(W + 1);
        d.grid = s->d_grid = s->alloc_internal<gd::GridHdr>(W);
        d.rgrid = s->d_rgrid = s->alloc_internal<gd::GridHdr>(W);
        d.knn_prev = s->alloc_internal<float4>(WA);
        d.road_bbox = s->d_road_bbox = s->alloc_internal<float4>(W);
        d.road_rbmax = s->d_road_rbmax = s->alloc_internal<float>(W);
        d.bev_dirty = s->alloc_internal<int32_t>(WA);
        d.bev_list = s->alloc_internal<int32_t>(WA);
        d.bev_count = s->alloc_internal<int32_t>(2);
        d.bev_all_dirty = 0;
        HIP_CHECK(hipMemset(d.bev_dirty, 1, sizeof(int32_t) * WA));  // (non-zero: everything is to be rasterised until k_world_step says otherwise)
        d.lidar_dirty = s->alloc_internal<int32_t>(WA);
        d.lidar_head = s->alloc_internal<float>(WA);
        HIP_CHECK(hipMemset(d.lidar_dirty, 1, sizeof(int32_t) * WA));
        HIP_CHECK(hipMemset(d.lidar_head, 0xff, sizeof(float) * WA));
        d.lin_apw = 2;
        if (const char *e = std::getenv("GPUDRIVE_LIN_AGENTS_PER_WAVE")) d.lin_apw = std::min(A / 4, std::max(1, std::atoi(e)));
        // worst case: every class as long as the longest one, which holds at most W / 8 + a few worlds' agents
        s->lin_cap = (static_cast<size_t>(W) + 64) * static_cast<size_t>(A) + 8 * 4 * static_cast<size_t>(d.lin_apw) + 64;
        s->d_lin_list = s->alloc_internal<int32_t>(s->lin_cap);
        s->d_lin_list_dyn = s->alloc_internal<int32_t>(s->lin_cap);
        d.lin_list = s->d_lin_list; d.lin_list_dyn = s->d_lin_list_dyn;
        d.lin_blocks = 0; d.lin_blocks_dyn = 0; d.lin_dyn_off = 0;
        d.lin_on = std::getenv("GPUDRIVE_LINEAR_LEGACY") == nullptr ? 1 : 0;
        d.pose_stamp = s->alloc_internal<uint4>(WA);
        d.pose_skip = std::getenv("GPUDRIVE_NO_POSE_SKIP") == nullptr ? 1 : 0;
        d.stat_skipped = s->alloc_internal<unsigned long long>(GD_SKIP_SLOTS);
        s->d_row_of_slot = s->alloc_internal<int32_t>(WA);
        s->d_slot_of_row = s->alloc_internal<int32_t>(WA);
        s->d_row_count = s->alloc_internal<int32_t>(1);
        d.bad_actions = s->alloc_internal<unsigned long long>(1);
        d.blk_off = s->d_blk_off = s->alloc_internal<int32_t>(W + 1);
        d.warm_k = 0;
        d.warm_all = 0;
        d.warm_flags = s->alloc_internal<int32_t>(W);
        d.warm_count = s->alloc_internal<unsigned long long>(1);
        // rank replay of the reference-order selection (map_obs_rank.hip): a fallback group is one workgroup of k_map_obs.
        // Its buffers (7.4 KB per agent slot) are allocated when a batch first takes the path (rebuild_worlds).
        d.rk_on = 0;
        d.rk_dbg = 0;
        d.rk_min_roads = 1536;
        // GPUDRIVE_RANK_WAVES pins the workgroups of the standard ranking launch (rounded up to a multiple of 8, one share per
        // XCD): few waves that take many turns each on the small worlds of a test
        d.rk_waves = 0;
        if (const char *e = std::getenv("GPUDRIVE_RANK_WAVES")) d.rk_waves = std::min(std::max((std::atoi(e) + 7) / 8 * 8, 8), GD_RANK_GRID);
        // GPUDRIVE_RANK_SCAN_ROWS=1: k_knn_scan writes a checkpoint row for every ranked agent and workgroup b takes world b,
        // as before the ranking read an agent's own checkpoints itself (A/B runs; the twin of tests/test_gpu_rank_setup.py)
        d.rk_scan_rows = 0;
        if (const char *e = std::getenv("GPUDRIVE_RANK_SCAN_ROWS")) d.rk_scan_rows = std::atoi(e) != 0 ? 1 : 0;
        // GPUDRIVE_RANK_SCAN_KERNEL=1: the set-up of the selection (rank_setup.hpp) as k_knn_scan's launch behind the state step,
        // as before k_world_step ran it itself (A/B runs; the twin of tests/test_gpu_rank_fold.py)
        d.rk_scan_kernel = 0;
        if (const char *e = std::getenv("GPUDRIVE_RANK_SCAN_KERNEL")) d.rk_scan_kernel = std::atoi(e) != 0 ? 1 : 0;
        // where a list of the standard ranking is drawn from its cursor, the waves the device holds at a time empty it: those
        // behind them (the launch has a wave per live agent, up to GD_RANK_GRID) leave without asking
        d.rk_resident = std::max(gd::rank_resident_waves(A) / 8, 1);
        s->rk_possible = GD_MAP_OBS_AW == 32 && cfg->knn_order != GD_KNN_SET_ORDER &&
                         params->roadObservationAlgorithm == GD_ROADS_K_NEAREST && std::getenv("GPUDRIVE_NO_RANK_REPLAY") == nullptr;
#ifdef GD_DIAG
        if (const char *e = std::getenv("GPUDRIVE_RANK_DBG")) d.rk_dbg = std::atoi(e);
#endif
        for (int i = 0; i < gd_sim::kRing; i++) {
            void *pinned = nullptr;
            HIP_CHECK(hipHostMalloc(&pinned, sizeof(int32_t) * W, hipHostMallocDefault));
            s->h_flags[i].reset(static_cast<int32_t *>(pinned));
            s->flag_ev[i] = make_event(hipEventDisableTiming);
        }
        std::vector<int> all(W);
        for (int w = 0; w < W; w++) all[w] = w;
        s->rebuild_worlds(all);
        // Sim::Sim -> initWorld for every world, then Manager::reset({}) (src/sim.cpp:1008-1011, src/mgr.cpp:565)
        s->do_reset(std::vector<int32_t>(W, 1));
        HIP_CHECK(hipStreamSynchronize(s->stream));
    });
    if (rc != GD_OK) return rc;
    *out = s.release();
    return GD_OK;
}

void gd_destroy(gd_sim *sim) { delete sim; }

int gd_step(gd_sim *s) {
    if (!s) return fail(GD_ERR_INVALID, "gd_step: null sim");
    return guarded([&]() { s->step(); });
}

int gd_reset(gd_sim *s, const int32_t *idx, int32_t n) {
    if (!s || (n > 0 && !idx)) return fail(GD_ERR_INVALID, "gd_reset: bad argument");
    std::vector<int32_t> flags(s->W, 0);
    for (int i = 0; i < n; i++) {
        if (idx[i] < 0 || idx[i] >= s->W) return fail(GD_ERR_INVALID, "gd_reset: world index out of range");
        flags[idx[i]] = 1;
    }
    return guarded([&]() { s->do_reset(flags); });
}

int gd_set_maps(gd_sim *s, const char *const *scenes, int32_t n) {
    if (!s || !scenes) return fail(GD_ERR_INVALID, "gd_set_maps: null argument");
    if (n != s->W) return fail(GD_ERR_INVALID, "gd_set_maps: len(maps) must equal the number of worlds");
    const std::vector<std::string> old_scenes = s->scenes;
    const std::vector<int32_t> old_deleted = s->deleted;
    const int rc = guarded([&]() {
        for (int w = 0; w < n; w++) {
            if (!scenes[w]) throw std::invalid_argument("gd_set_maps: null scene path");
            s->scenes[w] = scenes[w];
        }
        std::fill(s->deleted.begin(), s->deleted.end(), -1);  // src/mgr.cpp:613-617
        std::vector<int> all(s->W);
        for (int w = 0; w < s->W; w++) all[w] = w;
        s->rebuild_worlds(all);
        s->do_reset(std::vector<int32_t>(s->W, 1));
    });
    if (rc != GD_OK && rc != GD_ERR_DEVICE) {  // leave the previous worlds in place on a bad file
        s->scenes = old_scenes;
        s->deleted = old_deleted;
    }
    return rc;
}

int gd_delete_agents(gd_sim *s, const int32_t *worlds, const int32_t *offsets, const int32_t *ids, int32_t nw) {
    if (!s || (nw > 0 && (!worlds || !offsets))) return fail(GD_ERR_INVALID, "gd_delete_agents: null argument");
    std::vector<int> touched;
    for (int i = 0; i < nw; i++) {
        const int w = worlds[i], cnt = offsets[i + 1] - offsets[i];
        if (w < 0 || w >= s->W) return fail(GD_ERR_INVALID, "gd_delete_agents: world index out of range");
        if (cnt < 0 || cnt > s->A) return fail(GD_ERR_INVALID, "gd_delete_agents: too many ids for one world");
    }
    return guarded([&]() {
        for (int i = 0; i < nw; i++) {
            const int w = worlds[i], cnt = offsets[i + 1] - offsets[i];
            for (int k = 0; k < cnt; k++) s->deleted[static_cast<size_t>(w) * s->A + k] = ids[offsets[i] + k];
            touched.push_back(w);
        }
        s->rebuild_worlds(touched);
        s->do_reset(std::vector<int32_t>(s->W, 1));  // src/mgr.cpp:712-714: reset(all)
    });
}

int gd_tensor(gd_sim *s, int32_t id, gd_tensor_desc *out) {
    if (!s || !out || id < 0 || id >= GD_T_COUNT) return fail(GD_ERR_INVALID, "gd_tensor: bad argument");
    if (!s->exported[id]) return fail(GD_ERR_UNSUPPORTED, "tensor not allocated (set gd_config.alloc_bev for the BEV tensor)");
    gd_tensor_shape(id, s->W, s->A, out);
    out->data = s->exported[id];
    return GD_OK;
}

int gd_pack_observations(gd_sim *s, float *out, int64_t out_bytes) {
    if (!s || !out) return fail(GD_ERR_INVALID, "gd_pack_observations: null argument");
    const int64_t D = 6 + static_cast<int64_t>(s->A - 1) * 6 + GD_MAP_OBS_K * 13;
    const int64_t need = static_cast<int64_t>(s->W) * s->A * D * 4;
    if (out_bytes < need) return fail(GD_ERR_INVALID, "gd_pack_observations: output buffer too small");
    if (s->d.pack && s->d.pack_rows && s->d.pack_only)
        return fail(GD_ERR_UNSUPPORTED, "gd_pack_observations: learner rows are attached with only = 1: the raw rows are stale");
    return guarded([&]() {
        if (s->d.pack && !s->d.pack_rows) {  // the step already wrote it (gd_attach_packed): nothing to do, or a copy for another buffer
            if (out != s->d.pack) HIP_CHECK(hipMemcpyAsync(out, s->d.pack, need, hipMemcpyDeviceToDevice, s->stream));
            return;
        }
        gd::launch_pack_obs(s->d, s->stream, out);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_attach_packed(gd_sim *s, float *out, int64_t out_bytes, int32_t only) {
    if (!s) return fail(GD_ERR_INVALID, "gd_attach_packed: null sim");
    const int64_t D = 6 + static_cast<int64_t>(s->A - 1) * 6 + GD_MAP_OBS_K * 13;
    if (out && out_bytes < static_cast<int64_t>(s->W) * s->A * D * 4)
        return fail(GD_ERR_INVALID, "gd_attach_packed: output buffer too small");
    if (out && !s->direct_pack_supported())
        return fail(GD_ERR_UNSUPPORTED, "gd_attach_packed: not available with disableClassicalObs or GPUDRIVE_LINEAR_LEGACY=1: use gd_pack_observations");
    return guarded([&]() {
        if (!out) s->detach_packed();  // (either kind)
        else s->attach_packed(out, only != 0, false);
    });
}

int gd_set_learner_rows(gd_sim *s, const uint8_t *mask, int32_t n_rows) {
    if (!s) return fail(GD_ERR_INVALID, "gd_set_learner_rows: null sim");
    const size_t WA = static_cast<size_t>(s->W) * s->A;
    if (mask && (n_rows < 0 || static_cast<size_t>(n_rows) > WA))
        return fail(GD_ERR_INVALID, "gd_set_learner_rows: n_rows out of range");
    int32_t count = 0;
    const int rc = guarded([&]() {
        if (s->d.pack && s->d.pack_rows) s->detach_packed();  // its rows belong to the previous map
        HIP_CHECK(hipStreamSynchronize(s->stream));
        s->drop_graph();
        s->d.row_of_slot = nullptr;
        s->d.slot_of_row = nullptr;
        s->d.n_rows = 0;
        if (!mask) return;
        gd::launch_learner_rows(s->stream, mask, WA, s->d_row_of_slot, s->d_slot_of_row, s->d_row_count);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(&count, s->d_row_count, sizeof(count), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
    });
    if (rc != GD_OK || !mask) return rc;
    if (count != n_rows) return fail(GD_ERR_INVALID, "gd_set_learner_rows: n_rows differs from the number of true slots of the mask");
    s->d.row_of_slot = s->d_row_of_slot;
    s->d.slot_of_row = s->d_slot_of_row;
    s->d.n_rows = count;
    return GD_OK;
}

int gd_attach_packed_rows(gd_sim *s, float *out, int64_t out_bytes, int32_t only) {
    if (!s || !out) return fail(GD_ERR_INVALID, "gd_attach_packed_rows: null argument (gd_attach_packed(sim, NULL, 0, 0) detaches)");
    if (!s->d.row_of_slot) return fail(GD_ERR_INVALID, "gd_attach_packed_rows: no learner rows set (gd_set_learner_rows)");
    const int64_t D = 6 + static_cast<int64_t>(s->A - 1) * 6 + GD_MAP_OBS_K * 13;
    if (out_bytes < static_cast<int64_t>(s->d.n_rows) * D * 4) return fail(GD_ERR_INVALID, "gd_attach_packed_rows: output buffer too small");
    if (!s->direct_pack_supported())
        return fail(GD_ERR_UNSUPPORTED, "gd_attach_packed_rows: not available with disableClassicalObs or GPUDRIVE_LINEAR_LEGACY=1");
    return guarded([&]() { s->attach_packed(out, only != 0, true); });
}

int gd_attach_packed_rows_conditioned(gd_sim *s, float *out, int64_t out_bytes, int32_t only, const float *weights) {
    if (!s || !out || !weights)
        return fail(GD_ERR_INVALID, "gd_attach_packed_rows_conditioned: null argument (gd_attach_packed(sim, NULL, 0, 0) detaches)");
    if (!s->d.row_of_slot) return fail(GD_ERR_INVALID, "gd_attach_packed_rows_conditioned: no learner rows set (gd_set_learner_rows)");
    const int64_t R = 6 + static_cast<int64_t>(s->A - 1) * 6 + GD_MAP_OBS_K * 13 + 3;
    if (out_bytes < static_cast<int64_t>(s->d.n_rows) * R * 4)
        return fail(GD_ERR_INVALID, "gd_attach_packed_rows_conditioned: output buffer too small");
    if (!s->direct_pack_supported())
        return fail(GD_ERR_UNSUPPORTED, "gd_attach_packed_rows_conditioned: not available with disableClassicalObs or GPUDRIVE_LINEAR_LEGACY=1");
    return guarded([&]() { s->attach_packed(out, only != 0, true, weights); });
}

int gd_set_discrete_actions(gd_sim *s, const int64_t *indices, const float *table, int32_t n_actions) {
    if (!s) return fail(GD_ERR_INVALID, "gd_set_discrete_actions: null sim");
    if (s->d.p.dynamicsModel == GD_DYNAMICS_STATE)
        return fail(GD_ERR_UNSUPPORTED, "gd_set_discrete_actions: the State dynamics model has no discrete action space");
    if (!s->d.row_of_slot) return fail(GD_ERR_INVALID, "gd_set_discrete_actions: no learner rows set (gd_set_learner_rows)");
    if (n_actions < 0 || (s->d.n_rows > 0 && (!indices || !table)))
        return fail(GD_ERR_INVALID, "gd_set_discrete_actions: bad argument");
    return guarded([&]() {
        gd::launch_discrete_actions(s->d, s->stream, indices, table, n_actions);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_pack_observations_conditioned(gd_sim *s, const float *weights, float *out, int64_t out_bytes) {
    if (!s || !weights || !out) return fail(GD_ERR_INVALID, "gd_pack_observations_conditioned: null argument");
    const int64_t R = 6 + static_cast<int64_t>(s->A - 1) * 6 + GD_MAP_OBS_K * 13 + 3;
    if (out_bytes < static_cast<int64_t>(s->W) * s->A * R * 4)
        return fail(GD_ERR_INVALID, "gd_pack_observations_conditioned: output buffer too small");
    if (s->d.pack && s->d.pack_rows && s->d.pack_only)
        return fail(GD_ERR_UNSUPPORTED, "gd_pack_observations_conditioned: learner rows are attached with only = 1: the raw rows are stale");
    return guarded([&]() {
        gd::launch_pack_obs_conditioned(s->d, s->stream, weights, out);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_expert_actions(gd_sim *s, float *actions, int32_t action_cols, float *pos_xy, float *vel_xy, float *yaw,
                      int32_t *valids) {
    if (!s) return fail(GD_ERR_INVALID, "gd_expert_actions: null sim");
    const int cols = s->d.p.dynamicsModel == GD_DYNAMICS_STATE ? 10 : 3;
    if (actions && action_cols != cols)
        return fail(GD_ERR_INVALID, "gd_expert_actions: action_cols does not match the dynamics model (10 for State, else 3)");
    return guarded([&]() {
        gd::launch_expert_actions(s->d, s->stream, actions, pos_xy, vel_xy, yaw, valids);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_advance_log_playback(gd_sim *s, int32_t init_steps) {
    if (!s) return fail(GD_ERR_INVALID, "gd_advance_log_playback: null sim");
    if (init_steps < 0 || init_steps >= GD_EPISODE_LEN)
        return fail(GD_ERR_INVALID, "gd_advance_log_playback: the expert trajectory has 91 steps, init_steps must be < 91");
    return guarded([&]() {
        for (int t = 0; t < init_steps; t++) {
            gd::launch_set_log_actions(s->d, s->stream, t);
            HIP_CHECK(hipGetLastError());
            s->step();
        }
    });
}

int gd_record_expert(gd_sim *s, const gd_record_buffers *b, int32_t n_steps) {
    if (!s || !b) return fail(GD_ERR_INVALID, "gd_record_expert: null argument");
    if (!b->row_slot || !b->obs || !b->actions || !b->dead_mask || !b->partner_mask || !b->road_mask || !b->ego_global_pos ||
        !b->ego_global_rot || !b->dead || !b->goal_achieved || !b->off_road || !b->veh_collision || !b->any_alive)
        return fail(GD_ERR_INVALID, "gd_record_expert: every buffer is required");
    if (b->n_rows < 0) return fail(GD_ERR_INVALID, "gd_record_expert: n_rows must be >= 0");
    if (n_steps < 1 || n_steps > GD_EPISODE_LEN)
        return fail(GD_ERR_INVALID, "gd_record_expert: the expert trajectory has 91 steps, n_steps must be in [1, 91]");
    if (s->d.p.dynamicsModel == GD_DYNAMICS_STATE)
        return fail(GD_ERR_INVALID, "gd_record_expert: the State dynamics model's actions have 10 columns, the dataset's have 3");
    if (s->d.pack && s->d.pack_only)
        return fail(GD_ERR_UNSUPPORTED, "gd_record_expert: a packed buffer is attached with only = 1: the raw rows are stale");
    return guarded([&]() {
        std::vector<Event> ev;  // the optional diagnostic: a pair around every recorder launch
        auto mark = [&]() {
            if (!b->kernel_ms) return;
            ev.push_back(make_event());
            HIP_CHECK(hipEventRecord(ev.back().get(), s->stream));
        };
        for (int t = 0; t <= n_steps; t++) {
            mark();
            gd::launch_record(s->d, s->stream, *b, t, t < n_steps);
            HIP_CHECK(hipGetLastError());
            mark();
            if (t == n_steps) break;
            gd::launch_set_log_actions(s->d, s->stream, t);
            HIP_CHECK(hipGetLastError());
            s->step();
        }
        if (b->kernel_ms) {
            HIP_CHECK(hipStreamSynchronize(s->stream));
            float sum = 0.f;
            for (size_t i = 0; i + 1 < ev.size(); i += 2) {
                float ms = 0.f;
                HIP_CHECK(hipEventElapsedTime(&ms, ev[i].get(), ev[i + 1].get()));
                sum += ms;
            }
            *b->kernel_ms = sum;
        }
    });
}

namespace {

// what gd_il_index and gd_il_batch both require of the dataset table; rows: the source rows of every shard together
const char *il_dataset_error(const gd_il_dataset *ds, int64_t *rows) {
    if (!ds) return "null argument";
    if (ds->max_agents != 64 && ds->max_agents != 128) return "max_agents must be 64 or 128";
    if (ds->rollout_len < 1 || ds->pred_len < 1 || ds->rollout_len + ds->pred_len > GD_EPISODE_LEN)
        return "rollout_len >= 1, pred_len >= 1 and rollout_len + pred_len <= 91 are required";
    if (ds->n_shards < 0 || ds->n_shards > GD_IL_MAX_SHARDS) return "0 to 8 shards";
    *rows = 0;
    for (int i = 0; i < ds->n_shards; i++) {
        const gd_il_shard &sh = ds->shard[i];
        if (sh.n_rows < 0) return "a shard's n_rows must be >= 0";
        if (!sh.obs || !sh.actions || !sh.dead_mask || !sh.partner_mask || !sh.road_mask || !sh.keep)
            return "every array of every shard is required";
        if (reinterpret_cast<uintptr_t>(sh.obs) % 16 != 0 || reinterpret_cast<uintptr_t>(sh.road_mask) % 8 != 0)
            return "obs must be 16-byte aligned and road_mask 8-byte aligned";
        *rows += sh.n_rows;
    }
    if (*rows > INT32_MAX / GD_EPISODE_LEN) return "too many rows";
    return nullptr;
}

}  // namespace

int gd_il_index(const gd_il_dataset *ds, int32_t *counts, int32_t *kept, const int64_t *entry_offset, const int64_t *kept_ordinal,
                int32_t *entries, void *stream) {
    int64_t rows = 0;
    if (const char *e = il_dataset_error(ds, &rows)) return fail(GD_ERR_INVALID, std::string("gd_il_index: ") + e);
    if (entries ? (!entry_offset || !kept_ordinal) : (!counts || !kept))
        return fail(GD_ERR_INVALID, "gd_il_index: counts and kept (first launch) or entry_offset, kept_ordinal and entries "
                                    "(second launch) are required");
    return guarded([&]() {
        gd::launch_il_index(*ds, static_cast<hipStream_t>(stream), rows, counts, kept, entry_offset, kept_ordinal, entries);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_il_batch(const gd_il_dataset *ds, const gd_il_batch_buffers *b, void *stream) {
    int64_t rows = 0;
    if (const char *e = il_dataset_error(ds, &rows)) return fail(GD_ERR_INVALID, std::string("gd_il_batch: ") + e);
    if (!b) return fail(GD_ERR_INVALID, "gd_il_batch: null argument");
    if (b->batch < 0 || b->n_entries < 0) return fail(GD_ERR_INVALID, "gd_il_batch: batch and n_entries must be >= 0");
    if (b->batch > INT32_MAX / 64) return fail(GD_ERR_INVALID, "gd_il_batch: batch too large for one launch");
    if (!b->entries || !b->sel || !b->bad_indices || !b->obs || !b->actions || !b->partner_mask || !b->road_mask || !b->data_idx)
        return fail(GD_ERR_INVALID, "gd_il_batch: every buffer is required");
    if (reinterpret_cast<uintptr_t>(b->obs) % 16 != 0 || reinterpret_cast<uintptr_t>(b->road_mask) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(b->entries) % 16 != 0)
        return fail(GD_ERR_INVALID, "gd_il_batch: obs and entries must be 16-byte aligned and road_mask 8-byte aligned");
    // developer switch for the sweep tools/il_batches.py records (NOTEBOOK.md): workgroups per sample
    int split = 0;
    if (const char *e = std::getenv("GPUDRIVE_IL_SPLIT")) split = std::min(64, std::max(1, std::atoi(e)));
    return guarded([&]() {
        gd::launch_il_batch(*ds, static_cast<hipStream_t>(stream), *b, split);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_il_future_batch(const gd_il_dataset *ds, const gd_il_future *fu, const gd_il_future_buffers *b, void *stream) {
    int64_t rows = 0;
    if (const char *e = il_dataset_error(ds, &rows)) return fail(GD_ERR_INVALID, std::string("gd_il_future_batch: ") + e);
    if (!fu || !b) return fail(GD_ERR_INVALID, "gd_il_future_batch: null argument");
    if (fu->future_step < 1 || fu->future_step > GD_EPISODE_LEN - 1)
        return fail(GD_ERR_INVALID, "gd_il_future_batch: future_step must be 1..90");
    if (fu->exp != GD_IL_FUTURE_OTHER && fu->exp != GD_IL_FUTURE_EGO) return fail(GD_ERR_INVALID, "gd_il_future_batch: unknown exp");
    for (const double *edges : {fu->xbins, fu->ybins})
        for (int i = 0; i < 9; i++)
            if (!std::isfinite(edges[i]) || (i && !(edges[i - 1] < edges[i])))
                return fail(GD_ERR_INVALID, "gd_il_future_batch: the bin edges must be finite and strictly increasing");
    for (int i = 0; i < ds->n_shards; i++)
        if (!fu->ego_global_pos[i] || !fu->ego_global_rot[i])
            return fail(GD_ERR_INVALID, "gd_il_future_batch: ego_global_pos and ego_global_rot of every shard are required");
    if (b->batch < 0 || b->n_entries < 0) return fail(GD_ERR_INVALID, "gd_il_future_batch: batch and n_entries must be >= 0");
    if (b->batch > INT32_MAX / 64) return fail(GD_ERR_INVALID, "gd_il_future_batch: batch too large for one launch");
    if (!b->entries || !b->sel || !b->bad_indices || !b->obs || !b->actions || !b->valid_mask || !b->ego_mask || !b->partner_mask ||
        !b->road_mask || !b->future_mask || !b->future_pos)
        return fail(GD_ERR_INVALID, "gd_il_future_batch: every buffer is required");
    if (reinterpret_cast<uintptr_t>(b->obs) % 16 != 0 || reinterpret_cast<uintptr_t>(b->road_mask) % 8 != 0 ||
        reinterpret_cast<uintptr_t>(b->entries) % 16 != 0 || reinterpret_cast<uintptr_t>(b->future_pos) % 8 != 0)
        return fail(GD_ERR_INVALID, "gd_il_future_batch: obs and entries must be 16-byte aligned, road_mask and future_pos "
                                    "8-byte aligned");
    int split = 0;  // (gd_il_batch's developer switch)
    if (const char *e = std::getenv("GPUDRIVE_IL_SPLIT")) split = std::min(64, std::max(1, std::atoi(e)));
    return guarded([&]() {
        gd::launch_il_future(*ds, *fu, static_cast<hipStream_t>(stream), *b, split);
        HIP_CHECK(hipGetLastError());
    });
}

namespace {

bool misaligned(const void *p, size_t n) { return reinterpret_cast<uintptr_t>(p) % n != 0; }

// what every gd_rollout_* entry point requires of the buffer table
const char *rollout_error(const gd_rollout *ro) {
    if (!ro) return "null argument";
    if (ro->batch_size < 1 || ro->num_rows < 1 || ro->obs_width < 1 || ro->action_width < 1)
        return "batch_size, num_rows, obs_width and action_width must be >= 1";
    if (ro->num_rows > (1 << 20)) return "num_rows above 2^20";
    if (ro->batch_size > (1 << 22)) return "batch_size above 2^22";
    if ((int64_t)ro->batch_size * std::max(ro->obs_width, ro->action_width) > ((int64_t)1 << 40)) return "storage above 2^40 elements";
    if (!ro->obs || !ro->actions || !ro->logprobs || !ro->rewards || !ro->dones || !ro->values || !ro->row || !ro->ord ||
        !ro->count || !ro->dst || !ro->state)
        return "every buffer is required";
    if (misaligned(ro->actions, 8)) return "actions must be 8-byte aligned";
    for (const void *p : {(const void *)ro->obs, (const void *)ro->logprobs, (const void *)ro->rewards, (const void *)ro->dones,
                          (const void *)ro->values, (const void *)ro->row, (const void *)ro->ord, (const void *)ro->count,
                          (const void *)ro->dst, (const void *)ro->state})
        if (misaligned(p, 4)) return "float and int32 buffers must be 4-byte aligned";
    return nullptr;
}

}  // namespace

int gd_rollout_store(const gd_rollout *ro, const float *obs, const float *value, const int64_t *action, const float *logprob,
                     const float *reward, const uint8_t *done, const uint8_t *mask, int32_t streaming, void *stream) {
    if (const char *e = rollout_error(ro)) return fail(GD_ERR_INVALID, std::string("gd_rollout_store: ") + e);
    if (!obs || !value || !action || !logprob || !reward || !done || !mask)
        return fail(GD_ERR_INVALID, "gd_rollout_store: every input is required");
    if (misaligned(obs, 4) || misaligned(value, 4) || misaligned(logprob, 4) || misaligned(reward, 4) || misaligned(action, 8))
        return fail(GD_ERR_INVALID, "gd_rollout_store: float inputs must be 4-byte aligned and action 8-byte aligned");
    return guarded([&]() {
        gd::launch_rollout_store(*ro, static_cast<hipStream_t>(stream), obs, value, action, logprob, reward, done, mask,
                                 streaming != 0);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_rollout_sort(const gd_rollout *ro, const int64_t *offset, int64_t *idxs, void *stream) {
    if (const char *e = rollout_error(ro)) return fail(GD_ERR_INVALID, std::string("gd_rollout_sort: ") + e);
    if (!offset || !idxs) return fail(GD_ERR_INVALID, "gd_rollout_sort: offset and idxs are required");
    if (misaligned(offset, 8) || misaligned(idxs, 8)) return fail(GD_ERR_INVALID, "gd_rollout_sort: offset and idxs must be 8-byte aligned");
    return guarded([&]() {
        gd::launch_rollout_sort(*ro, static_cast<hipStream_t>(stream), offset, idxs);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_rollout_gae(const gd_rollout *ro, const int64_t *idxs, float gamma, float gae_lambda, float *delta, float *coef,
                   float *advantages, void *stream) {
    if (const char *e = rollout_error(ro)) return fail(GD_ERR_INVALID, std::string("gd_rollout_gae: ") + e);
    if (!idxs || !delta || !coef || !advantages) return fail(GD_ERR_INVALID, "gd_rollout_gae: every buffer is required");
    if (misaligned(idxs, 8) || misaligned(delta, 4) || misaligned(coef, 4) || misaligned(advantages, 4))
        return fail(GD_ERR_INVALID, "gd_rollout_gae: idxs must be 8-byte aligned, delta, coef and advantages 4-byte aligned");
    if (!std::isfinite(gamma) || !std::isfinite(gae_lambda) || !std::isfinite(gamma * gae_lambda))
        return fail(GD_ERR_INVALID, "gd_rollout_gae: gamma, gae_lambda and their product must be finite");
    return guarded([&]() {
        gd::launch_rollout_gae(*ro, static_cast<hipStream_t>(stream), idxs, gamma, gae_lambda, delta, coef, advantages);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_rollout_gather(const gd_rollout *ro, const gd_rollout_batch *b, void *stream) {
    if (const char *e = rollout_error(ro)) return fail(GD_ERR_INVALID, std::string("gd_rollout_gather: ") + e);
    if (!b) return fail(GD_ERR_INVALID, "gd_rollout_gather: null argument");
    if (b->num_minibatches < 1 || b->minibatch_rows < 1 || b->bptt_horizon < 1 ||
        (int64_t)b->num_minibatches * b->minibatch_rows * b->bptt_horizon != ro->batch_size)
        return fail(GD_ERR_INVALID, "gd_rollout_gather: num_minibatches * minibatch_rows * bptt_horizon must be batch_size");
    if (b->first < 0 || b->n < 1 || b->n > b->num_minibatches - b->first)
        return fail(GD_ERR_INVALID, "gd_rollout_gather: [first, first + n) must lie inside the minibatches");
    if (b->split < 0 || b->split > 64) return fail(GD_ERR_INVALID, "gd_rollout_gather: split must be 0..64");
    // one launch of 256-lane workgroups: samples * split workgroups must stay below 2^24 (2^32 lanes)
    if ((int64_t)b->n * b->minibatch_rows * b->bptt_horizon * std::max(b->split, 1) >= ((int64_t)1 << 24))
        return fail(GD_ERR_INVALID, "gd_rollout_gather: samples * split must be below 2^24");
    if (!b->idxs || !b->advantages || !b->obs || !b->actions || !b->logprobs || !b->dones || !b->values || !b->advantages_out ||
        !b->returns)
        return fail(GD_ERR_INVALID, "gd_rollout_gather: every buffer is required");
    if (misaligned(b->idxs, 8) || misaligned(b->actions, 8) || misaligned(b->advantages, 4) || misaligned(b->obs, 4) ||
        misaligned(b->logprobs, 4) || misaligned(b->dones, 4) || misaligned(b->values, 4) || misaligned(b->advantages_out, 4) ||
        misaligned(b->returns, 4))
        return fail(GD_ERR_INVALID, "gd_rollout_gather: idxs and actions must be 8-byte aligned, float buffers 4-byte aligned");
    return guarded([&]() {
        gd::launch_rollout_gather(*ro, static_cast<hipStream_t>(stream), *b);
        HIP_CHECK(hipGetLastError());
    });
}

// everything gd_policy_forward refuses; nullptr when everything is in order
static const char *policy_forward_problem(const gd_policy *p, const float *obs, const float *u, int32_t deterministic,
                                          const int64_t *actions, const float *logprob, const float *entropy, const float *value,
                                          const float *logits_out) {
    if (!p || !obs || !actions || !logprob || !entropy || !value || (!u && !deterministic)) return "null argument";
    if (p->max_agents != 64 && p->max_agents != 128) return "max_agents must be 64 or 128";
    if (p->ego_width != 6 && p->ego_width != 9) return "ego_width must be 6 or 9";
    if (p->n_actions < 1 || p->n_actions > 1024) return "n_actions must be in [1, 1024]";
    if (p->num_rows < 1 || p->num_rows > (1 << 20)) return "num_rows must be in [1, 2^20]";
    if (!p->blob || !p->features || !p->logits) return "blob, features and logits are required";
    if (p->blob_floats != gd::policy_blob_floats(p->ego_width, p->n_actions))
        return "blob_floats is not the layout's size for this ego_width and n_actions";
    if (misaligned(p->blob, 16) || misaligned(p->features, 16)) return "blob and features must be 16-byte aligned";
    if (misaligned(actions, 8) || misaligned(obs, 4) || (u && misaligned(u, 4)) || misaligned(p->logits, 4) || misaligned(logprob, 4) ||
        misaligned(entropy, 4) || misaligned(value, 4) || (logits_out && misaligned(logits_out, 4)))
        return "actions must be 8-byte aligned, float buffers 4-byte aligned";
    return nullptr;
}

int gd_policy_forward(const gd_policy *p, const float *obs, const float *u, int32_t deterministic, int64_t *actions,
                      float *logprob, float *entropy, float *value, float *logits_out, void *stream) {
    if (const char *why = policy_forward_problem(p, obs, u, deterministic, actions, logprob, entropy, value, logits_out))
        return fail(GD_ERR_INVALID, std::string("gd_policy_forward: ") + why);
    return guarded([&]() {
        gd::launch_policy_forward(*p, static_cast<hipStream_t>(stream), obs, u, deterministic != 0, actions, logprob, entropy, value,
                                  logits_out);
        HIP_CHECK(hipGetLastError());
    });
}

// the checks gd_policy_evaluate and gd_policy_backward share; nullptr when everything is in order
static const char *policy_grad_problem(const gd_policy *p, const gd_policy_grad *g) {
    if (p->max_agents != 64 && p->max_agents != 128) return "max_agents must be 64 or 128";
    if (p->ego_width != 6 && p->ego_width != 9) return "ego_width must be 6 or 9";
    if (p->n_actions < 1 || p->n_actions > 1024) return "n_actions must be in [1, 1024]";
    if (p->num_rows < 1 || p->num_rows > (1 << 20)) return "num_rows must be in [1, 2^20]";
    if (!g->features || !g->logits || !g->winners) return "features, logits and winners are required";
    if (misaligned(g->features, 16) || misaligned(g->logits, 4)) return "features must be 16-byte aligned, logits 4-byte aligned";
    return nullptr;
}

// everything gd_policy_evaluate refuses; nullptr when everything is in order
static const char *policy_evaluate_problem(const gd_policy *p, const gd_policy_grad *g, const float *obs, const int64_t *actions,
                                           const float *logprob, const float *entropy, const float *value) {
    if (!p || !g || !obs || !actions || !logprob || !entropy || !value) return "null argument";
    if (const char *why = policy_grad_problem(p, g)) return why;
    if (!p->blob) return "blob is required";
    if (p->blob_floats != gd::policy_blob_floats(p->ego_width, p->n_actions))
        return "blob_floats is not the layout's size for this ego_width and n_actions";
    if (misaligned(p->blob, 16)) return "blob must be 16-byte aligned";
    if (misaligned(actions, 8) || misaligned(obs, 4) || misaligned(logprob, 4) || misaligned(entropy, 4) || misaligned(value, 4))
        return "actions must be 8-byte aligned, float buffers 4-byte aligned";
    return nullptr;
}

int gd_policy_evaluate(const gd_policy *p, const gd_policy_grad *g, const float *obs, const int64_t *actions, float *logprob,
                       float *entropy, float *value, void *stream) {
    if (const char *why = policy_evaluate_problem(p, g, obs, actions, logprob, entropy, value))
        return fail(GD_ERR_INVALID, std::string("gd_policy_evaluate: ") + why);
    return guarded([&]() {
        gd_policy q = *p;
        q.features = g->features, q.logits = g->logits;
        gd::launch_policy_evaluate(q, static_cast<hipStream_t>(stream), obs, actions, g->winners, logprob, entropy, value);
        HIP_CHECK(hipGetLastError());
    });
}

// everything gd_policy_backward refuses; nullptr when everything is in order
static const char *policy_backward_problem(const gd_policy *p, const gd_policy_grad *g, const float *obs, const int64_t *actions,
                                           const float *d_logprob, const float *d_entropy, const float *d_value,
                                           const float *grad) {
    if (!p || !g || !obs || !actions || !d_logprob || !d_entropy || !d_value || !grad) return "null argument";
    if (const char *why = policy_grad_problem(p, g)) return why;
    if (!g->params || !g->rowstat || !g->partials) return "params, rowstat and partials are required";
    if (g->num_partials < 1 || g->num_partials > 1024) return "num_partials must be in [1, 1024]";
    if (g->grad_floats != gd::policy_grad_floats(p->ego_width, p->n_actions))
        return "grad_floats is not the parameter count for this ego_width and n_actions";
    if (misaligned(actions, 8) || misaligned(obs, 4) || misaligned(d_logprob, 4) || misaligned(d_entropy, 4) || misaligned(d_value, 4) ||
        misaligned(grad, 4) || misaligned(g->params, 4) || misaligned(g->rowstat, 4) || misaligned(g->partials, 4))
        return "actions must be 8-byte aligned, float buffers 4-byte aligned";
    return nullptr;
}

int gd_policy_backward(const gd_policy *p, const gd_policy_grad *g, const float *obs, const int64_t *actions,
                       const float *d_logprob, const float *d_entropy, const float *d_value, float *grad, void *stream) {
    if (const char *why = policy_backward_problem(p, g, obs, actions, d_logprob, d_entropy, d_value, grad))
        return fail(GD_ERR_INVALID, std::string("gd_policy_backward: ") + why);
    return guarded([&]() {
        gd::launch_policy_backward(*p, *g, static_cast<hipStream_t>(stream), obs, actions, d_logprob, d_entropy, d_value, grad);
        HIP_CHECK(hipGetLastError());
    });
}

// everything gd_ppo_loss refuses; nullptr when everything is in order
static const char *ppo_loss_problem(const gd_ppo *o, const float *newlogprob, const float *entropy, const float *newvalue,
                                    const float *old_logprob, const float *old_value, const float *adv, const float *ret,
                                    const float *d_logprob, const float *d_entropy, const float *d_value) {
    if (!o || !newlogprob || !entropy || !newvalue || !old_logprob || !old_value || !adv || !ret || !d_logprob || !d_entropy ||
        !d_value)
        return "null argument";
    if (o->num_rows < 1 || o->num_rows > (1 << 20)) return "num_rows must be in [1, 2^20]";
    if (o->norm_adv && o->num_rows < 2) return "norm_adv needs at least two rows (the unbiased variance of one is undefined)";
    if (!o->stats || !o->stats_sum) return "stats and stats_sum are required";
    if (misaligned(newlogprob, 4) || misaligned(entropy, 4) || misaligned(newvalue, 4) || misaligned(old_logprob, 4) ||
        misaligned(old_value, 4) || misaligned(adv, 4) || misaligned(ret, 4) || misaligned(d_logprob, 4) ||
        misaligned(d_entropy, 4) || misaligned(d_value, 4) || misaligned(o->stats, 4) || misaligned(o->stats_sum, 4))
        return "float buffers must be 4-byte aligned";
    return nullptr;
}

int gd_ppo_loss(const gd_ppo *ppo, const float *newlogprob, const float *entropy, const float *newvalue, const float *old_logprob,
                const float *old_value, const float *adv, const float *ret, float *d_logprob, float *d_entropy, float *d_value,
                void *stream) {
    if (const char *why = ppo_loss_problem(ppo, newlogprob, entropy, newvalue, old_logprob, old_value, adv, ret, d_logprob, d_entropy,
                                           d_value))
        return fail(GD_ERR_INVALID, std::string("gd_ppo_loss: ") + why);
    return guarded([&]() {
        gd::launch_ppo_loss(*ppo, static_cast<hipStream_t>(stream), newlogprob, entropy, newvalue, old_logprob, old_value, adv, ret,
                            d_logprob, d_entropy, d_value);
        HIP_CHECK(hipGetLastError());
    });
}

// everything gd_ppo_adam refuses; nullptr when everything is in order
static const char *ppo_adam_problem(const gd_ppo *o, const float *grad) {
    if (!o || !grad) return "null argument";
    if (o->ego_width != 6 && o->ego_width != 9) return "ego_width must be 6 or 9";
    if (o->n_actions < 1 || o->n_actions > 1024) return "n_actions must be in [1, 1024]";
    if (o->grad_floats != gd::policy_grad_floats(o->ego_width, o->n_actions))
        return "grad_floats is not the parameter count for this ego_width and n_actions";
    if (o->blob_floats != gd::policy_blob_floats(o->ego_width, o->n_actions))
        return "blob_floats is not the layout's size for this ego_width and n_actions";
    if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0)) return "betas must be in [0, 1)";
    if (!(o->eps > 0.f) || !(o->max_grad_norm > 0.f)) return "eps and max_grad_norm must be positive";
    if (!o->lr || !o->step || !o->beta_pow || !o->params || !o->exp_avg || !o->exp_avg_sq || !o->blob || !o->blob_of || !o->stats ||
        !o->stats_sum || !o->scal)
        return "lr, step, beta_pow, params, exp_avg, exp_avg_sq, blob, blob_of, stats, stats_sum and scal are required";
    if (misaligned(o->beta_pow, 8) || misaligned(grad, 4) || misaligned(o->lr, 4) || misaligned(o->step, 4) || misaligned(o->params, 4) ||
        misaligned(o->exp_avg, 4) || misaligned(o->exp_avg_sq, 4) || misaligned(o->blob, 4) || misaligned(o->blob_of, 4) ||
        misaligned(o->stats, 4) || misaligned(o->stats_sum, 4) || misaligned(o->scal, 4))
        return "beta_pow must be 8-byte aligned, the other buffers 4-byte aligned";
    return nullptr;
}

int gd_ppo_adam(const gd_ppo *ppo, const float *grad, void *stream) {
    if (const char *why = ppo_adam_problem(ppo, grad)) return fail(GD_ERR_INVALID, std::string("gd_ppo_adam: ") + why);
    return guarded([&]() {
        gd::launch_ppo_adam(*ppo, static_cast<hipStream_t>(stream), grad);
        HIP_CHECK(hipGetLastError());
    });
}

// everything gd_ppo_update refuses of non-null p, g and ppo; nullptr when everything is in order
static const char *ppo_update_problem(const gd_policy *p, const gd_policy_grad *g, const gd_ppo *ppo, const float *obs,
                                      const int64_t *actions, const float *old_logprob, const float *old_value, const float *adv,
                                      const float *ret) {
    const gd_ppo &o = *ppo;
    const char *why = policy_evaluate_problem(p, g, obs, actions, o.newlogprob, o.entropy, o.newvalue);
    if (!why) why = ppo_loss_problem(ppo, o.newlogprob, o.entropy, o.newvalue, old_logprob, old_value, adv, ret, o.d_logprob,
                                     o.d_entropy, o.d_value);
    if (!why) why = policy_backward_problem(p, g, obs, actions, o.d_logprob, o.d_entropy, o.d_value, o.grad);
    if (!why) why = ppo_adam_problem(ppo, o.grad);
    if (!why && (p->num_rows != o.num_rows || p->ego_width != o.ego_width || p->n_actions != o.n_actions))
        why = "num_rows, ego_width and n_actions of the policy and of ppo differ";
    if (!why && (p->blob != o.blob || g->params != o.params))
        why = "the policy's blob and params must be ppo's (the optimiser step updates both in place)";
    return why;
}

int gd_ppo_update(const gd_policy *p, const gd_policy_grad *g, const gd_ppo *ppo, const float *obs, const int64_t *actions,
                  const float *old_logprob, const float *old_value, const float *adv, const float *ret, void *stream) {
    if (!p || !g || !ppo) return fail(GD_ERR_INVALID, "gd_ppo_update: null argument");
    const gd_ppo &o = *ppo;
    if (const char *why = ppo_update_problem(p, g, ppo, obs, actions, old_logprob, old_value, adv, ret))
        return fail(GD_ERR_INVALID, std::string("gd_ppo_update: ") + why);
    return guarded([&]() {
        hipStream_t st = static_cast<hipStream_t>(stream);
        gd_policy q = *p;
        q.features = g->features, q.logits = g->logits;
        gd::launch_policy_evaluate(q, st, obs, actions, g->winners, o.newlogprob, o.entropy, o.newvalue);
        gd::launch_ppo_loss(o, st, o.newlogprob, o.entropy, o.newvalue, old_logprob, old_value, adv, ret, o.d_logprob, o.d_entropy,
                            o.d_value);
        gd::launch_policy_backward(*p, *g, st, obs, actions, o.d_logprob, o.d_entropy, o.d_value, o.grad);
        gd::launch_ppo_adam(o, st, o.grad);
        HIP_CHECK(hipGetLastError());
    });
}

// everything the *_dropout calls refuse of d; nullptr when everything is in order
static const char *dropout_problem(const gd_dropout *d) {
    if (!d->call || !d->used) return "dropout: call and used are required";
    if (misaligned(d->call, 8) || misaligned(d->used, 8)) return "dropout: call and used must be 8-byte aligned";
    if (d->threshold < 1 || d->threshold > 65535) return "dropout: threshold must be in [1, 65535]";
    if (!std::isfinite(d->scale)) return "dropout: scale must be finite";
    return nullptr;
}

int gd_policy_forward_dropout(const gd_policy *p, const gd_dropout *d, const float *obs, const float *u, int32_t deterministic,
                              int64_t *actions, float *logprob, float *entropy, float *value, float *logits_out, void *stream) {
    if (!d) return gd_policy_forward(p, obs, u, deterministic, actions, logprob, entropy, value, logits_out, stream);
    const char *why = policy_forward_problem(p, obs, u, deterministic, actions, logprob, entropy, value, logits_out);
    if (!why) why = dropout_problem(d);
    if (why) return fail(GD_ERR_INVALID, std::string("gd_policy_forward_dropout: ") + why);
    return guarded([&]() {
        gd::launch_policy_forward(*p, *d, static_cast<hipStream_t>(stream), obs, u, deterministic != 0, actions, logprob, entropy,
                                  value, logits_out);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_policy_evaluate_dropout(const gd_policy *p, const gd_policy_grad *g, const gd_dropout *d, const float *obs,
                               const int64_t *actions, float *logprob, float *entropy, float *value, void *stream) {
    if (!d) return gd_policy_evaluate(p, g, obs, actions, logprob, entropy, value, stream);
    const char *why = policy_evaluate_problem(p, g, obs, actions, logprob, entropy, value);
    if (!why) why = dropout_problem(d);
    if (why) return fail(GD_ERR_INVALID, std::string("gd_policy_evaluate_dropout: ") + why);
    return guarded([&]() {
        gd_policy q = *p;
        q.features = g->features, q.logits = g->logits;
        gd::launch_policy_evaluate(q, *d, static_cast<hipStream_t>(stream), obs, actions, g->winners, logprob, entropy, value);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_policy_backward_dropout(const gd_policy *p, const gd_policy_grad *g, const gd_dropout *d, const float *obs,
                               const int64_t *actions, const float *d_logprob, const float *d_entropy, const float *d_value,
                               float *grad, void *stream) {
    if (!d) return gd_policy_backward(p, g, obs, actions, d_logprob, d_entropy, d_value, grad, stream);
    const char *why = policy_backward_problem(p, g, obs, actions, d_logprob, d_entropy, d_value, grad);
    if (!why) why = dropout_problem(d);
    if (why) return fail(GD_ERR_INVALID, std::string("gd_policy_backward_dropout: ") + why);
    return guarded([&]() {
        gd::launch_policy_backward(*p, *g, *d, static_cast<hipStream_t>(stream), obs, actions, d_logprob, d_entropy, d_value, grad);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_ppo_update_dropout(const gd_policy *p, const gd_policy_grad *g, const gd_ppo *ppo, const gd_dropout *d, const float *obs,
                          const int64_t *actions, const float *old_logprob, const float *old_value, const float *adv,
                          const float *ret, void *stream) {
    if (!d) return gd_ppo_update(p, g, ppo, obs, actions, old_logprob, old_value, adv, ret, stream);
    if (!p || !g || !ppo) return fail(GD_ERR_INVALID, "gd_ppo_update_dropout: null argument");
    const gd_ppo &o = *ppo;
    const char *why = ppo_update_problem(p, g, ppo, obs, actions, old_logprob, old_value, adv, ret);
    if (!why) why = dropout_problem(d);
    if (why) return fail(GD_ERR_INVALID, std::string("gd_ppo_update_dropout: ") + why);
    return guarded([&]() {
        hipStream_t st = static_cast<hipStream_t>(stream);
        gd_policy q = *p;
        q.features = g->features, q.logits = g->logits;
        gd::launch_policy_evaluate(q, *d, st, obs, actions, g->winners, o.newlogprob, o.entropy, o.newvalue);
        gd::launch_ppo_loss(o, st, o.newlogprob, o.entropy, o.newvalue, old_logprob, old_value, adv, ret, o.d_logprob, o.d_entropy,
                            o.d_value);
        gd::launch_policy_backward(*p, *g, *d, st, obs, actions, o.d_logprob, o.d_entropy, o.d_value, o.grad);
        gd::launch_ppo_adam(o, st, o.grad);
        HIP_CHECK(hipGetLastError());
    });
}

// everything the calls that take a row list refuse of it; nullptr when everything is in order
static const char *row_list_problem(const int32_t *rows, const int32_t *count) {
    if (!rows || !count) return "rows and count are required";
    if (misaligned(rows, 4) || misaligned(count, 4)) return "rows and count must be 4-byte aligned";
    return nullptr;
}

// everything the closed loops refuse of their list of live rows (gd_bc_rollout_rows, gd_policy_rollout_rows: the same fields)
static const char *rollout_rows_problem(const int32_t *rows, const int32_t *count, const int32_t *scratch, const int32_t *live_count,
                                        int32_t reserved) {
    if (const char *why = row_list_problem(rows, count)) return why;
    if (!scratch || misaligned(scratch, 4)) return "scratch is required and must be 4-byte aligned";
    if (misaligned(live_count, 4)) return "live_count must be 4-byte aligned";
    if (reserved != 0) return "the row list's reserved must be 0";
    return nullptr;
}

// everything the BC forward refuses at network_dim dim (64 or 128), whoever calls it; nullptr when everything is in order
static const char *bc_forward_problem(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                                      int32_t n, int32_t deterministic, const float *u, const float *z, const float *expert_actions,
                                      const gd_bc_outputs *out, int dim) {
    if (!p || !obs || !partner_mask || !road_mask || !out) return "null argument";
    if (!deterministic && (!u || !z)) return "u and z are required unless deterministic";
    if (out->nll && !expert_actions) return "expert_actions is required with out->nll";
    if (p->max_agents != 64 && p->max_agents != 128) return "max_agents must be 64 or 128";
    if (p->num_stack < 1 || p->num_stack > 8) return "num_stack must be in [1, 8]";
    if (p->fusion_layers < 1 || p->fusion_layers > 4 || p->branch_layers < 1 || p->branch_layers > 4)
        return "fusion_layers and branch_layers must be in [1, 4]";
    if (p->head_layers < 0 || p->head_layers > 4) return "head_layers must be in [0, 4]";
    if (p->n_components < 1 || p->n_components > 16) return "n_components must be in [1, 16]";
    if (!(p->clip_value == p->clip_value)) return "clip_value must not be NaN";
    if (p->chunk_rows < 1 || p->chunk_rows > 4096) return "chunk_rows must be in [1, 4096]";
    if (n < 1 || n > (1 << 20)) return "n must be in [1, 2^20]";
    if (!p->blob || !p->scratch) return "blob and scratch are required";
    if (p->blob_floats != gd::bc_blob_floats(dim, p->num_stack, p->fusion_layers, p->branch_layers, p->head_layers, p->n_components))
        return dim == 128 ? "blob_floats is not the layout's size at network_dim 128 for these layer counts, num_stack and n_components"
                          : "blob_floats is not the layout's size for these layer counts, num_stack and n_components";
    if (p->scratch_floats < gd::bc_scratch_floats(dim, p->max_agents, p->chunk_rows))
        return dim == 128 ? "scratch_floats is below chunk_rows * 3 * (max_agents + 200) * 128"
                          : "scratch_floats is below chunk_rows * 3 * (max_agents + 200) * 64";
    if (misaligned(p->blob, 16) || misaligned(p->scratch, 256)) return "blob must be 16-byte aligned, scratch 256-byte aligned";
    if (misaligned(obs, 4) || (u && misaligned(u, 4)) || (z && misaligned(z, 4)) || (expert_actions && misaligned(expert_actions, 4)) ||
        misaligned(out->context, 4) || misaligned(out->means, 4) || misaligned(out->log_covariances, 4) ||
        misaligned(out->covariances, 4) || misaligned(out->weights, 4) || misaligned(out->actions, 4) || misaligned(out->nll, 4) ||
        misaligned(out->ego_attn_score, 4) || misaligned(out->component, 4))
        return "float and int32 buffers must be 4-byte aligned";
    return nullptr;
}

// everything of a gd_bc_readout that the entries with one refuse (the policy has passed bc_forward_problem); nullptr when
// everything is in order
static const char *bc_readout_problem(const gd_bc_policy *p, const gd_bc_readout *r) {
    if (!r) return "readout is required";
    if (r->tap != GD_LP_TAP_FUSION && r->tap != GD_LP_TAP_RO) return "readout: tap must be GD_LP_TAP_FUSION or GD_LP_TAP_RO";
    if (r->layer < 0 || r->layer >= (r->tap == GD_LP_TAP_RO ? p->branch_layers : p->fusion_layers))
        return "readout: layer must be in [0, layers of the tapped block)";
    if (r->n_other < 0 || r->n_other > GD_BC_READOUT_MAX || r->n_ego < 0 || r->n_ego > GD_BC_READOUT_MAX)
        return "readout: n_other and n_ego must be in [0, 8]";
    if (r->n_other + r->n_ego < 1) return "readout: at least one probe is required";
    if (r->reserved != 0) return "readout: reserved must be 0";
    if (r->intervene != 0 && r->intervene != 1) return "readout: intervene must be 0 or 1";
    if (r->intervene && (r->n_other != r->n_ego)) return "readout: intervene needs n_other == n_ego";
    for (int i = 0; i < r->n_other; i++) {
        if (!r->other[i].packed || misaligned(r->other[i].packed, 16)) return "readout: a probe's packed is required, 16-byte aligned";
        if (r->intervene && (!r->other[i].weight || misaligned(r->other[i].weight, 4)))
            return "readout: an 'other' probe's weight is required with intervene, 4-byte aligned";
    }
    for (int i = 0; i < r->n_ego; i++)
        if (!r->ego[i].packed || misaligned(r->ego[i].packed, 16)) return "readout: a probe's packed is required, 16-byte aligned";
    if ((r->n_other && !r->other_pred) || (r->n_ego && !r->ego_pred) || (r->intervene && !r->ego_pred_prime))
        return "readout: an output of a non-zero count is null";
    if ((r->n_other && r->other_stride < (int64_t)r->n_other * (p->max_agents - 1)) || (r->n_ego && r->ego_stride < r->n_ego) ||
        (r->intervene && r->prime_stride < r->n_ego))
        return "readout: a stride is below its row";
    if (misaligned(r->labels, 8)) return "readout: labels must be 8-byte aligned";
    if (r->intervene && (!r->bad_labels || misaligned(r->bad_labels, 4)))
        return "readout: bad_labels is required with intervene, 4-byte aligned";
    return nullptr;
}

// what the *_dim entry points refuse of the struct itself, before its base is looked at; nullptr when it is in order
static const char *bc_dim_problem(const gd_bc_policy_dim *p) {
    if (!p) return "null argument";
    if (p->network_dim != 64 && p->network_dim != 128) return "network_dim must be 64 or 128";
    if (p->reserved != 0) return "reserved must be 0";
    return nullptr;
}

// The policy and the width an entry runs at: a gd_bc_policy is 64 wide, a gd_bc_policy_dim says its own.  why: bc_dim_problem's
// answer, with which dim is not to be used; p is NULL only where the entry's own argument is.
struct BCAt {
    const gd_bc_policy *p;
    int dim;
    const char *why;
};
static BCAt bc_at(const gd_bc_policy *p) { return {p, 64, nullptr}; }
static BCAt bc_at(const gd_bc_policy_dim *p) { return {p ? &p->base : nullptr, p ? p->network_dim : 0, bc_dim_problem(p)}; }

// what an entry takes beside the arguments every entry of its family has
enum { BC_READOUT = 1, BC_ROWS = 2 };

// The one checked forward behind the six gd_bc_forward* entries.  takes: the read-out and / or the row list, which the entry
// then requires (their own checks refuse a NULL); an entry that takes none passes none.  The order of refusal is every entry's:
// the _dim struct, the policy and the buffers at its width, the read-out, the row list.
static int bc_forward(const char *who, int takes, BCAt at, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                      int32_t n, int32_t deterministic, const float *u, const float *z, const float *expert_actions,
                      const gd_bc_outputs *out, const gd_bc_readout *readout, const int32_t *rows, const int32_t *count, void *stream) {
    const char *why = at.why;
    if (!why) why = bc_forward_problem(at.p, obs, partner_mask, road_mask, n, deterministic, u, z, expert_actions, out, at.dim);
    if (!why && (takes & BC_READOUT)) why = bc_readout_problem(at.p, readout);
    if (!why && (takes & BC_ROWS)) why = row_list_problem(rows, count);
    if (why) return fail(GD_ERR_INVALID, std::string(who) + ": " + why);
    return guarded([&]() {
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (takes & BC_ROWS)
            gd::launch_bc_forward_rows(*at.p, at.dim, st, obs, partner_mask, road_mask, n, deterministic != 0, u, z, expert_actions, *out,
                                       rows, count, readout);
        else
            gd::launch_bc_forward(*at.p, at.dim, st, obs, partner_mask, road_mask, n, deterministic != 0, u, z, expert_actions, *out,
                                  readout);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_bc_forward(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                  int32_t deterministic, const float *u, const float *z, const float *expert_actions, const gd_bc_outputs *out,
                  void *stream) {
    return bc_forward("gd_bc_forward", 0, bc_at(p), obs, partner_mask, road_mask, n, deterministic, u, z, expert_actions, out, nullptr,
                      nullptr, nullptr, stream);
}

int gd_bc_forward_rows(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                       int32_t deterministic, const float *u, const float *z, const float *expert_actions, const gd_bc_outputs *out,
                       const int32_t *rows, const int32_t *count, void *stream) {
    return bc_forward("gd_bc_forward_rows", BC_ROWS, bc_at(p), obs, partner_mask, road_mask, n, deterministic, u, z, expert_actions, out,
                      nullptr, rows, count, stream);
}

int gd_bc_forward_readout(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                          int32_t deterministic, const float *u, const float *z, const float *expert_actions, const gd_bc_outputs *out,
                          const gd_bc_readout *readout, void *stream) {
    return bc_forward("gd_bc_forward_readout", BC_READOUT, bc_at(p), obs, partner_mask, road_mask, n, deterministic, u, z,
                      expert_actions, out, readout, nullptr, nullptr, stream);
}

int gd_bc_forward_rows_readout(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                               int32_t n, int32_t deterministic, const float *u, const float *z, const float *expert_actions,
                               const gd_bc_outputs *out, const gd_bc_readout *readout, const int32_t *rows, const int32_t *count,
                               void *stream) {
    return bc_forward("gd_bc_forward_rows_readout", BC_READOUT | BC_ROWS, bc_at(p), obs, partner_mask, road_mask, n, deterministic, u, z,
                      expert_actions, out, readout, rows, count, stream);
}

int gd_bc_forward_dim(const gd_bc_policy_dim *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                      int32_t deterministic, const float *u, const float *z, const float *expert_actions, const gd_bc_outputs *out,
                      void *stream) {
    return bc_forward("gd_bc_forward_dim", 0, bc_at(p), obs, partner_mask, road_mask, n, deterministic, u, z, expert_actions, out,
                      nullptr, nullptr, nullptr, stream);
}

int gd_bc_forward_rows_dim(const gd_bc_policy_dim *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                           int32_t n, int32_t deterministic, const float *u, const float *z, const float *expert_actions,
                           const gd_bc_outputs *out, const int32_t *rows, const int32_t *count, void *stream) {
    return bc_forward("gd_bc_forward_rows_dim", BC_ROWS, bc_at(p), obs, partner_mask, road_mask, n, deterministic, u, z, expert_actions,
                      out, nullptr, rows, count, stream);
}

// everything the closed loop refuses of the simulator, the buffers and the policy at network_dim dim (none of them NULL); GD_OK
// when everything is in order
static int bc_rollout_problem(const char *who, gd_sim *s, const gd_bc_policy *p, const gd_bc_rollout_buffers *b, int32_t n_steps,
                              int dim) {
    const std::string w = std::string(who) + ": ";
    if (!b->row_slot || !b->row_of_slot || !b->window || !b->partner_mask || !b->road_mask || !b->partner_value || !b->row_actions ||
        !b->dead || !b->goal_achieved || !b->off_road || !b->veh_collision || !b->goal_step || !b->off_road_step ||
        !b->init_goal_dist || !b->goal_dist || !b->any_alive || !b->summary)
        return fail(GD_ERR_INVALID, w + "every buffer but the per-step records is required");
    if (b->n_rows < 1 || b->n_rows > (1 << 20)) return fail(GD_ERR_INVALID, w + "n_rows must be in [1, 2^20]");
    if (n_steps < 1 || n_steps > GD_EPISODE_LEN)
        return fail(GD_ERR_INVALID, w + "an episode has 91 steps, n_steps must be in [1, 91]");
    if (s->d.p.dynamicsModel == GD_DYNAMICS_STATE)
        return fail(GD_ERR_INVALID, w + "the State dynamics model's actions have 10 columns, the policy's have 3");
    if (p->max_agents != s->A) return fail(GD_ERR_INVALID, w + "the policy's max_agents differs from the simulator's");
    gd_bc_outputs out{};
    out.actions = b->row_actions;
    if (const char *why = bc_forward_problem(p, b->window, b->partner_mask, b->road_mask, b->n_rows, b->deterministic, b->u, b->z,
                                             nullptr, &out, dim))
        return fail(GD_ERR_INVALID, w + why);
    if (misaligned(b->window, 16) || misaligned(b->goal_achieved, 4) || misaligned(b->off_road, 4) || misaligned(b->veh_collision, 4) ||
        misaligned(b->goal_step, 4) || misaligned(b->off_road_step, 4) || misaligned(b->init_goal_dist, 4) ||
        misaligned(b->goal_dist, 4) || misaligned(b->any_alive, 4) || misaligned(b->summary, 4) || misaligned(b->row_slot, 4) ||
        misaligned(b->row_of_slot, 4) || misaligned(b->actions, 4) || misaligned(b->ego_global_pos, 4) ||
        misaligned(b->ego_global_rot, 4))
        return fail(GD_ERR_INVALID, w + "window must be 16-byte aligned, float and int32 buffers 4-byte aligned");
    if (s->d.pack && s->d.pack_only)
        return fail(GD_ERR_UNSUPPORTED, w + "a packed buffer is attached with only = 1: the raw rows are stale");
    return GD_OK;
}

// The loop of every driver (bc_rollout.hip): r == nullptr is the forward on all N rows, otherwise the list of the rows with
// dead[n] == 0 in the loop.  When iteration t does not exist every row is dead: the list is empty and every workgroup of the
// forward returns at its first load.
// x: step t's forward also writes the step's slices of the read-outs; without the list the read-out kernel drops dead rows
// itself and one more launch zeroes the scores the head kernel stored for them.
// dim == 128: the wide forward in the same loop; there is no read-out at that width.
static int bc_rollout_run(gd_sim *s, const gd_bc_policy *p, const gd_bc_rollout_buffers *b, const gd_bc_rollout_rows *r,
                          int32_t n_steps, const gd_bc_rollout_reads *x, int dim) {
    return guarded([&]() {
        const size_t N = static_cast<size_t>(b->n_rows);
        gd_bc_outputs out{};
        out.actions = b->row_actions;
        const int score_row = 4 * (p->max_agents - 1);
        gd_bc_readout ro{};
        if (x && x->readout) ro = *x->readout;
        gd::launch_bc_rollout_post(s->d, s->stream, *b, -1, true);
        HIP_CHECK(hipGetLastError());
        for (int t = 0; t < n_steps; t++) {
            const float *u = b->u ? b->u + t * N : nullptr, *z = b->z ? b->z + t * N * 3 : nullptr;
            gd::launch_bc_rollout_row(s->d, s->stream, *b, t, p->num_stack);
            const gd_bc_readout *rd = nullptr;
            if (x) {
                out.ego_attn_score = x->ego_attn_score ? x->ego_attn_score + t * N * score_row : nullptr;
                if (x->readout) {
                    const gd_bc_readout &full = *x->readout;
                    ro.other_pred = full.other_pred ? full.other_pred + t * N * full.other_stride : nullptr;
                    ro.ego_pred = full.ego_pred ? full.ego_pred + t * N * full.ego_stride : nullptr;
                    ro.ego_pred_prime = full.ego_pred_prime ? full.ego_pred_prime + t * N * full.prime_stride : nullptr;
                    rd = &ro;
                }
            }
            if (r) {
                gd::launch_live_rows(s->stream, b->dead, b->n_rows, r->rows, r->count, r->scratch,
                                     r->live_count ? r->live_count + t : nullptr, true);
                gd::launch_bc_forward_rows(*p, dim, s->stream, b->window, b->partner_mask, b->road_mask, b->n_rows, b->deterministic != 0,
                                           u, z, nullptr, out, r->rows, r->count, rd);
            } else {
                gd::launch_bc_forward(*p, dim, s->stream, b->window, b->partner_mask, b->road_mask, b->n_rows, b->deterministic != 0, u, z,
                                      nullptr, out, rd, b->dead);
                if (out.ego_attn_score) gd::launch_bc_rollout_score_fill(s->stream, *b, out.ego_attn_score, score_row);
            }
            gd::launch_bc_rollout_actions(s->d, s->stream, *b, t);
            HIP_CHECK(hipGetLastError());
            s->step();
            gd::launch_bc_rollout_post(s->d, s->stream, *b, t, t + 1 < n_steps);
            HIP_CHECK(hipGetLastError());
        }
        gd::launch_bc_rollout_summary(s->stream, *b);
        HIP_CHECK(hipGetLastError());
    });
}

// The one checked loop behind the four gd_bc_rollout* entries.  takes: the list (r) and / or the reads (x) the entry refuses to
// go without; both are optional otherwise.  What needs no simulator is checked first: the _dim struct, the list, the reads.
static int bc_rollout(const char *who, int takes, gd_sim *s, BCAt at, const gd_bc_rollout_buffers *b, const gd_bc_rollout_rows *r,
                      const gd_bc_rollout_reads *x, int32_t n_steps) {
    const std::string w = std::string(who) + ": ";
    if (!s || !at.p || !b || ((takes & BC_ROWS) && !r) || ((takes & BC_READOUT) && !x))
        return fail(GD_ERR_INVALID, w + "null argument");
    const char *why = at.why;
    if (!why && r) why = rollout_rows_problem(r->rows, r->count, r->scratch, r->live_count, r->reserved);
    if (!why && x && !x->ego_attn_score && !x->readout) why = "reads needs ego_attn_score or readout";
    if (!why && x && misaligned(x->ego_attn_score, 4)) why = "ego_attn_score must be 4-byte aligned";
    if (!why && x && x->readout && at.dim != 64)
        why = "reads->readout must be NULL unless network_dim is 64 (the probes read 64-wide tokens)";
    if (why) return fail(GD_ERR_INVALID, w + why);
    if (const int rc = bc_rollout_problem(who, s, at.p, b, n_steps, at.dim)) return rc;
    if (x && x->readout)
        if (const char *bad = bc_readout_problem(at.p, x->readout)) return fail(GD_ERR_INVALID, w + bad);
    return bc_rollout_run(s, at.p, b, r, n_steps, x, at.dim);
}

// The closed-loop episode: gd_record_expert's loop with the policy where the logged action was.
int gd_bc_rollout(gd_sim *s, const gd_bc_policy *p, const gd_bc_rollout_buffers *b, int32_t n_steps) {
    return bc_rollout("gd_bc_rollout", 0, s, bc_at(p), b, nullptr, nullptr, n_steps);
}

// gd_bc_rollout with the list of live rows and gd_bc_forward_rows in the loop.
int gd_bc_rollout_compact(gd_sim *s, const gd_bc_policy *p, const gd_bc_rollout_buffers *b, const gd_bc_rollout_rows *r,
                          int32_t n_steps) {
    return bc_rollout("gd_bc_rollout_compact", BC_ROWS, s, bc_at(p), b, r, nullptr, n_steps);
}

// gd_bc_rollout (r == nullptr) or gd_bc_rollout_compact with the read-outs in the loop.
int gd_bc_rollout_readout(gd_sim *s, const gd_bc_policy *p, const gd_bc_rollout_buffers *b, const gd_bc_rollout_rows *r,
                          const gd_bc_rollout_reads *x, int32_t n_steps) {
    return bc_rollout("gd_bc_rollout_readout", BC_READOUT, s, bc_at(p), b, r, x, n_steps);
}

// gd_bc_rollout, gd_bc_rollout_compact (r) or gd_bc_rollout_readout (x) at the policy's width.
int gd_bc_rollout_dim(gd_sim *s, const gd_bc_policy_dim *p, const gd_bc_rollout_buffers *b, const gd_bc_rollout_rows *r,
                      const gd_bc_rollout_reads *x, int32_t n_steps) {
    return bc_rollout("gd_bc_rollout_dim", 0, s, bc_at(p), b, r, x, n_steps);
}

// everything gd_policy_rollout refuses, for gd_policy_rollout_compact too; GD_OK when everything is in order
static int policy_rollout_problem(const char *who, gd_sim *s, const gd_policy *p, const gd_policy_rollout_buffers *b, int32_t n_steps) {
    const std::string w = std::string(who) + ": ";
    if (!s || !p || !b) return fail(GD_ERR_INVALID, w + "null argument");
    if (!b->table || !b->actions || !b->logprob || !b->entropy || !b->value || !b->live || !b->goal_achieved || !b->collided ||
        !b->off_road || !b->world_active || !b->episode_lengths || !b->bad_indices || !b->any_active || !b->goal_achieved_count ||
        !b->frac_goal_achieved || !b->collided_count || !b->frac_collided || !b->off_road_count || !b->frac_off_road ||
        !b->other_count || !b->frac_other || !b->controlled_per_scene || !b->summary)
        return fail(GD_ERR_INVALID, w + "every buffer but u and the per-step records is required");
    if (b->n_rows < 1 || b->n_rows > (1 << 20)) return fail(GD_ERR_INVALID, w + "n_rows must be in [1, 2^20]");
    if (n_steps < 1 || n_steps > GD_EPISODE_LEN)
        return fail(GD_ERR_INVALID, w + "an episode has 91 steps, n_steps must be in [1, 91]");
    if (b->reserved != 0) return fail(GD_ERR_INVALID, w + "reserved must be 0");
    if (s->d.p.dynamicsModel == GD_DYNAMICS_STATE)
        return fail(GD_ERR_UNSUPPORTED, w + "the State dynamics model has no discrete action space");
    if (!s->d.row_of_slot) return fail(GD_ERR_INVALID, w + "no learner rows set (gd_set_learner_rows)");
    if (!s->d.pack || !s->d.pack_rows)
        return fail(GD_ERR_INVALID, w + "no learner-row buffer attached (gd_attach_packed_rows)");
    if (b->n_rows != s->d.n_rows) return fail(GD_ERR_INVALID, w + "n_rows differs from the number of learner rows");
    if (p->max_agents != s->A) return fail(GD_ERR_INVALID, w + "the policy's max_agents differs from the simulator's");
    if (p->ego_width != (s->d.pack_weights ? 9 : 6))
        return fail(GD_ERR_INVALID, w + "the policy's ego_width differs from the attached rows' (6, or 9 for conditioned rows)");
    if (p->num_rows != b->n_rows) return fail(GD_ERR_INVALID, w + "the policy's num_rows differs from n_rows");
    if (b->n_actions != p->n_actions) return fail(GD_ERR_INVALID, w + "the table's n_actions differs from the policy's");
    if (const char *why = policy_forward_problem(p, s->d.pack, b->u, b->deterministic, b->actions, b->logprob, b->entropy, b->value,
                                                 nullptr))
        return fail(GD_ERR_INVALID, w + why);
    if (misaligned(b->table, 4) || misaligned(b->goal_achieved, 4) || misaligned(b->collided, 4) || misaligned(b->off_road, 4) ||
        misaligned(b->episode_lengths, 4) || misaligned(b->bad_indices, 4) || misaligned(b->any_active, 4) ||
        misaligned(b->goal_achieved_count, 4) || misaligned(b->frac_goal_achieved, 4) || misaligned(b->collided_count, 4) ||
        misaligned(b->frac_collided, 4) || misaligned(b->off_road_count, 4) || misaligned(b->frac_off_road, 4) ||
        misaligned(b->other_count, 4) || misaligned(b->frac_other, 4) || misaligned(b->controlled_per_scene, 4) ||
        misaligned(b->summary, 4) || misaligned(b->actions_idx, 8) || misaligned(b->agent_positions, 4))
        return fail(GD_ERR_INVALID, w + "actions_idx must be 8-byte aligned, float and int32 buffers 4-byte aligned");
    return GD_OK;
}

// The loop of both evaluators: r == nullptr is gd_policy_rollout's forward on all N rows, otherwise the list in the loop.
static int policy_rollout_run(gd_sim *s, const gd_policy *p, const gd_policy_rollout_buffers *b, const gd_policy_rollout_rows *r,
                              int32_t n_steps) {
    return guarded([&]() {
        const size_t N = static_cast<size_t>(b->n_rows);
        for (int t = 0; t < n_steps; t++) {
            const float *u = b->u ? b->u + t * N : nullptr;
            if (r) {
                gd::launch_live_rows(s->stream, b->live, b->n_rows, r->rows, r->count, r->scratch,
                                     r->live_count ? r->live_count + t : nullptr);
                gd::launch_policy_forward_rows(*p, nullptr, s->stream, s->d.pack, u, b->deterministic != 0, b->actions, b->logprob,
                                               b->entropy, b->value, nullptr, r->rows, r->count);
            } else {
                gd::launch_policy_forward(*p, s->stream, s->d.pack, u, b->deterministic != 0, b->actions, b->logprob, b->entropy,
                                          b->value, nullptr);
            }
            gd::launch_policy_rollout_actions(s->d, s->stream, *b, t);
            HIP_CHECK(hipGetLastError());
            s->step();
            gd::launch_policy_rollout_book(s->d, s->stream, *b, t);
            HIP_CHECK(hipGetLastError());
        }
        gd::launch_policy_rollout_finish(s->d, s->stream, *b, n_steps);
        HIP_CHECK(hipGetLastError());
    });
}

// The closed-loop PPO evaluator (policy_rollout.hip): gd_bc_rollout's loop with the late-fusion policy on the learner rows.
int gd_policy_rollout(gd_sim *s, const gd_policy *p, const gd_policy_rollout_buffers *b, int32_t n_steps) {
    if (const int rc = policy_rollout_problem("gd_policy_rollout", s, p, b, n_steps)) return rc;
    return policy_rollout_run(s, p, b, nullptr, n_steps);
}

int gd_live_rows(const uint8_t *mask, int32_t n, int32_t *rows, int32_t *count, int32_t *scratch, void *stream) {
    if (!mask || !scratch) return fail(GD_ERR_INVALID, "gd_live_rows: null argument");
    if (const char *why = row_list_problem(rows, count)) return fail(GD_ERR_INVALID, std::string("gd_live_rows: ") + why);
    if (misaligned(scratch, 4)) return fail(GD_ERR_INVALID, "gd_live_rows: scratch must be 4-byte aligned");
    if (n < 1 || n > (1 << 20)) return fail(GD_ERR_INVALID, "gd_live_rows: n must be in [1, 2^20]");
    return guarded([&]() {
        gd::launch_live_rows(static_cast<hipStream_t>(stream), mask, n, rows, count, scratch, nullptr);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_policy_forward_rows(const gd_policy *p, const gd_dropout *d, const float *obs, const float *u, int32_t deterministic,
                           int64_t *actions, float *logprob, float *entropy, float *value, float *logits_out, const int32_t *rows,
                           const int32_t *count, void *stream) {
    const char *why = policy_forward_problem(p, obs, u, deterministic, actions, logprob, entropy, value, logits_out);
    if (!why && d) why = dropout_problem(d);
    if (!why) why = row_list_problem(rows, count);
    if (why) return fail(GD_ERR_INVALID, std::string("gd_policy_forward_rows: ") + why);
    return guarded([&]() {
        gd::launch_policy_forward_rows(*p, d, static_cast<hipStream_t>(stream), obs, u, deterministic != 0, actions, logprob, entropy,
                                       value, logits_out, rows, count);
        HIP_CHECK(hipGetLastError());
    });
}

// gd_policy_rollout with gd_live_rows and gd_policy_forward_rows in the loop.  The list is checked first: it needs no simulator.
int gd_policy_rollout_compact(gd_sim *s, const gd_policy *p, const gd_policy_rollout_buffers *b, const gd_policy_rollout_rows *r,
                              int32_t n_steps) {
    const char *who = "gd_policy_rollout_compact";
    if (!s || !p || !b || !r) return fail(GD_ERR_INVALID, std::string(who) + ": null argument");
    if (const char *why = rollout_rows_problem(r->rows, r->count, r->scratch, r->live_count, r->reserved)) return fail(GD_ERR_INVALID, std::string(who) + ": " + why);
    if (const int rc = policy_rollout_problem(who, s, p, b, n_steps)) return rc;
    return policy_rollout_run(s, p, b, r, n_steps);
}

// everything gd_owned_rows refuses; nullptr when everything is in order
static const char *owned_rows_problem(const uint8_t *mask, const uint8_t *owner, int32_t n, int32_t n_policies, const int32_t *rows,
                                      const int32_t *start, const int32_t *count, const int32_t *scratch, const int32_t *count_copy) {
    if (!mask || !owner || !rows || !start || !count || !scratch) return "null argument";
    if (misaligned(rows, 4) || misaligned(start, 4) || misaligned(count, 4) || misaligned(scratch, 4) || misaligned(count_copy, 4))
        return "rows, start, count, scratch and count_copy must be 4-byte aligned";
    if (n < 1 || n > (1 << 20)) return "n must be in [1, 2^20]";
    if (n_policies < 1 || n_policies > GD_POLICY_SET_MAX) return "n_policies must be in [1, 8]";
    return nullptr;
}

int gd_owned_rows(const uint8_t *mask, const uint8_t *owner, int32_t n, int32_t n_policies, int32_t *rows, int32_t *start,
                  int32_t *count, int32_t *scratch, int32_t *count_copy, void *stream) {
    if (const char *why = owned_rows_problem(mask, owner, n, n_policies, rows, start, count, scratch, count_copy))
        return fail(GD_ERR_INVALID, std::string("gd_owned_rows: ") + why);
    return guarded([&]() {
        gd::launch_owned_rows(static_cast<hipStream_t>(stream), mask, owner, n, n_policies, rows, start, count, scratch, count_copy);
        HIP_CHECK(hipGetLastError());
    });
}

// The set's policy i as the forward on an owned list runs it: the set's own scratch for the policy's.
static gd_policy set_policy(const gd_policy_set *set, int i) {
    gd_policy q = set->policy[i];
    q.features = set->features, q.logits = set->logits;
    return q;
}

// everything gd_policy_forward_owned refuses; nullptr when everything is in order
static const char *policy_set_problem(const gd_policy_set *set, const float *obs, const float *u, int32_t deterministic,
                                      const int64_t *actions, const float *logprob, const float *entropy, const float *value,
                                      const float *logits_out) {
    if (!set) return "null argument";
    if (set->n_policies < 1 || set->n_policies > GD_POLICY_SET_MAX) return "n_policies must be in [1, 8]";
    if (set->reserved != 0) return "the set's reserved must be 0";
    if (!set->features || !set->logits) return "the set's features and logits are required";
    for (int i = 0; i < set->n_policies; i++) {
        const gd_policy q = set_policy(set, i), &f = set->policy[0];
        if (const char *why = policy_forward_problem(&q, obs, u, deterministic, actions, logprob, entropy, value, logits_out))
            return why;
        if (q.num_rows != f.num_rows || q.max_agents != f.max_agents || q.ego_width != f.ego_width || q.n_actions != f.n_actions)
            return "the policies of a set must agree in num_rows, max_agents, ego_width and n_actions";
    }
    return nullptr;
}

static const char *owned_list_problem(const int32_t *rows, const int32_t *start, const int32_t *count) {
    if (!rows || !start || !count) return "rows, start and count are required";
    if (misaligned(rows, 4) || misaligned(start, 4) || misaligned(count, 4)) return "rows, start and count must be 4-byte aligned";
    return nullptr;
}

int gd_policy_forward_owned(const gd_policy_set *set, const float *obs, const float *u, int32_t deterministic, int64_t *actions,
                            float *logprob, float *entropy, float *value, float *logits_out, const int32_t *rows,
                            const int32_t *start, const int32_t *count, void *stream) {
    const char *why = policy_set_problem(set, obs, u, deterministic, actions, logprob, entropy, value, logits_out);
    if (!why) why = owned_list_problem(rows, start, count);
    if (why) return fail(GD_ERR_INVALID, std::string("gd_policy_forward_owned: ") + why);
    return guarded([&]() {
        gd::launch_policy_forward_owned(*set, static_cast<hipStream_t>(stream), obs, u, deterministic != 0, actions, logprob, entropy,
                                        value, logits_out, rows, start, count);
        HIP_CHECK(hipGetLastError());
    });
}

// The multi-policy evaluator: gd_policy_rollout_compact's loop with the owned list for the live list, then the per-policy
// metrics (multi_policy_rollout.hip).  The set and the list are checked first: they need no simulator.
int gd_multi_policy_rollout(gd_sim *s, const gd_policy_set *set, const gd_policy_rollout_buffers *b, const gd_multi_policy_buffers *m,
                            int32_t n_steps) {
    const std::string w = "gd_multi_policy_rollout: ";
    if (!s || !set || !b || !m) return fail(GD_ERR_INVALID, w + "null argument");
    if (set->n_policies < 1 || set->n_policies > GD_POLICY_SET_MAX) return fail(GD_ERR_INVALID, w + "n_policies must be in [1, 8]");
    const char *why = owned_rows_problem(b->live, m->owner, b->n_rows, set->n_policies, m->rows, m->start, m->count, m->scratch,
                                         m->list_count);
    if (!why && (!m->denominator || !m->goal_achieved_count || !m->frac_goal_achieved || !m->collided_count || !m->frac_collided ||
                 !m->off_road_count || !m->frac_off_road || !m->n_rows || !m->summary))
        why = "every buffer of gd_multi_policy_buffers but list_count is required";
    if (!why && (misaligned(m->denominator, 4) || misaligned(m->goal_achieved_count, 4) || misaligned(m->frac_goal_achieved, 4) ||
                 misaligned(m->collided_count, 4) || misaligned(m->frac_collided, 4) || misaligned(m->off_road_count, 4) ||
                 misaligned(m->frac_off_road, 4) || misaligned(m->n_rows, 4) || misaligned(m->summary, 4)))
        why = "the float buffers of gd_multi_policy_buffers must be 4-byte aligned";
    if (!why && m->reserved != 0) why = "the multi-policy buffers' reserved must be 0";
    if (why) return fail(GD_ERR_INVALID, w + why);
    const gd_policy first = set_policy(set, 0);
    if (const int rc = policy_rollout_problem("gd_multi_policy_rollout", s, &first, b, n_steps)) return rc;
    if ((why = policy_set_problem(set, s->d.pack, b->u, b->deterministic, b->actions, b->logprob, b->entropy, b->value, nullptr)))
        return fail(GD_ERR_INVALID, w + why);
    return guarded([&]() {
        const size_t N = static_cast<size_t>(b->n_rows);
        const int P = set->n_policies;
        for (int t = 0; t < n_steps; t++) {
            gd::launch_owned_rows(s->stream, b->live, m->owner, b->n_rows, P, m->rows, m->start, m->count, m->scratch,
                                  m->list_count ? m->list_count + t * P : nullptr);
            gd::launch_policy_forward_owned(*set, s->stream, s->d.pack, b->u ? b->u + t * N : nullptr, b->deterministic != 0,
                                            b->actions, b->logprob, b->entropy, b->value, nullptr, m->rows, m->start, m->count);
            gd::launch_policy_rollout_actions(s->d, s->stream, *b, t);
            HIP_CHECK(hipGetLastError());
            s->step();
            gd::launch_policy_rollout_book(s->d, s->stream, *b, t);
            HIP_CHECK(hipGetLastError());
        }
        gd::launch_policy_rollout_finish(s->d, s->stream, *b, n_steps);
        gd::launch_multi_policy_finish(s->d, s->stream, *b, *m, P);
        HIP_CHECK(hipGetLastError());
    });
}

// everything the BC backward refuses at network_dim dim (64 or 128), whoever calls it; nullptr when everything is in order
static const char *bc_backward_problem(const gd_bc_policy *p, const gd_bc_grad *g, const float *obs, const uint8_t *partner_mask,
                                       const uint8_t *road_mask, int32_t n, const float *expert_actions, const float *grad_nll,
                                       const float *nll, const float *grad, int dim) {
    const char *why = nullptr;
    gd_bc_outputs none{};
    if (!g || !expert_actions || !grad_nll || !grad)
        why = "null argument";
    else if ((why = bc_forward_problem(p, obs, partner_mask, road_mask, n, 1, nullptr, nullptr, expert_actions, &none, dim)))
        ;
    else if (g->num_partials < 1 || g->num_partials > 4096)
        why = "num_partials must be in [1, 4096]";
    else if (g->reserved != 0)
        why = "reserved must be 0";
    else if (!g->scratch || !g->partials)
        why = "scratch and partials are required";
    else if (g->grad_floats != gd::bc_grad_floats(dim, p->num_stack, p->fusion_layers, p->branch_layers, p->head_layers, p->n_components))
        why = dim == 128 ? "grad_floats is not the parameters' count at network_dim 128 for these layer counts, num_stack and n_components"
                         : "grad_floats is not the parameters' count for these layer counts, num_stack and n_components";
    else if (g->scratch_floats <
             gd::bc_grad_scratch_floats(dim, p->max_agents, p->chunk_rows, p->fusion_layers, p->branch_layers, p->blob_floats))
        why = dim == 128 ? "grad scratch_floats is below blob_floats rounded up to 64 + chunk_rows * (max_agents + 200) * (128 * "
                           "(fusion_layers + branch_layers + 5) + 16)"
                         : "grad scratch_floats is below blob_floats rounded up to 64 + chunk_rows * (max_agents + 200) * (64 * "
                           "(fusion_layers + branch_layers + 5) + 16)";
    else if (misaligned(g->scratch, 256) || misaligned(g->partials, 16) || misaligned(grad, 16))
        why = "grad scratch must be 256-byte aligned, partials and grad 16-byte aligned";
    else if (misaligned(grad_nll, 4) || misaligned(nll, 4))
        why = "float buffers must be 4-byte aligned";
    return why;
}

// The one checked backward behind gd_bc_backward and gd_bc_backward_dim.  The order of refusal: the _dim struct, then the
// policy, the buffers and the gradient's sizes at its width.
static int bc_backward(const char *who, BCAt at, const gd_bc_grad *g, const float *obs, const uint8_t *partner_mask,
                       const uint8_t *road_mask, int32_t n, const float *expert_actions, const float *grad_nll, float *nll, float *grad,
                       void *stream) {
    const char *why = at.why;
    if (!why) why = bc_backward_problem(at.p, g, obs, partner_mask, road_mask, n, expert_actions, grad_nll, nll, grad, at.dim);
    if (why) return fail(GD_ERR_INVALID, std::string(who) + ": " + why);
    return guarded([&]() {
        gd::launch_bc_backward(*at.p, at.dim, *g, static_cast<hipStream_t>(stream), obs, partner_mask, road_mask, n, expert_actions,
                               grad_nll, nll, grad);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_bc_backward(const gd_bc_policy *p, const gd_bc_grad *g, const float *obs, const uint8_t *partner_mask,
                   const uint8_t *road_mask, int32_t n, const float *expert_actions, const float *grad_nll, float *nll, float *grad,
                   void *stream) {
    return bc_backward("gd_bc_backward", bc_at(p), g, obs, partner_mask, road_mask, n, expert_actions, grad_nll, nll, grad, stream);
}

int gd_bc_backward_dim(const gd_bc_policy_dim *p, const gd_bc_grad *g, const float *obs, const uint8_t *partner_mask,
                       const uint8_t *road_mask, int32_t n, const float *expert_actions, const float *grad_nll, float *nll,
                       float *grad, void *stream) {
    return bc_backward("gd_bc_backward_dim", bc_at(p), g, obs, partner_mask, road_mask, n, expert_actions, grad_nll, nll, grad, stream);
}

// everything gd_bc_train_rows refuses; nullptr when everything is in order
static const char *bc_train_rows_problem(const gd_bc_opt *o, int32_t n, const float *nll, const float *actions,
                                         const float *expert_actions, const float *grad_nll) {
    if (!o || !nll || !actions || !expert_actions || !grad_nll) return "null argument";
    if (n < 1 || n > (1 << 20)) return "n must be in [1, 2^20]";
    if (!o->stats || !o->stats_sum) return "stats and stats_sum are required";
    if (misaligned(nll, 4) || misaligned(actions, 4) || misaligned(expert_actions, 4) || misaligned(grad_nll, 4) ||
        misaligned(o->stats, 4) || misaligned(o->stats_sum, 4))
        return "float buffers must be 4-byte aligned";
    return nullptr;
}

int gd_bc_train_rows(const gd_bc_opt *opt, int32_t n, const float *nll, const float *actions, const float *expert_actions,
                     float *grad_nll, void *stream) {
    if (const char *why = bc_train_rows_problem(opt, n, nll, actions, expert_actions, grad_nll))
        return fail(GD_ERR_INVALID, std::string("gd_bc_train_rows: ") + why);
    return guarded([&]() {
        gd::launch_bc_train_rows(*opt, static_cast<hipStream_t>(stream), n, nll, actions, expert_actions, grad_nll);
        HIP_CHECK(hipGetLastError());
    });
}

// everything gd_bc_adamw and gd_bc_adamw_dim refuse of opt and grad at network_dim dim (64 or 128); nullptr when everything is
// in order
static const char *bc_adamw_problem(const gd_bc_opt *o, const float *grad, int dim) {
    if (!o || !grad) return "null argument";
    if (o->num_stack < 1 || o->num_stack > 8) return "num_stack must be in [1, 8]";
    if (o->fusion_layers < 1 || o->fusion_layers > 4 || o->branch_layers < 1 || o->branch_layers > 4)
        return "fusion_layers and branch_layers must be in [1, 4]";
    if (o->head_layers < 0 || o->head_layers > 4) return "head_layers must be in [0, 4]";
    if (o->n_components < 1 || o->n_components > 16) return "n_components must be in [1, 16]";
    if (o->reserved != 0) return "reserved must be 0";
    if (o->grad_floats != gd::bc_grad_floats(dim, o->num_stack, o->fusion_layers, o->branch_layers, o->head_layers, o->n_components))
        return dim == 128 ? "grad_floats is not the parameters' count at network_dim 128 for these layer counts, num_stack and n_components"
                          : "grad_floats is not the parameters' count for these layer counts, num_stack and n_components";
    if (o->blob_floats != gd::bc_blob_floats(dim, o->num_stack, o->fusion_layers, o->branch_layers, o->head_layers, o->n_components))
        return dim == 128 ? "blob_floats is not the layout's size at network_dim 128 for these layer counts, num_stack and n_components"
                          : "blob_floats is not the layout's size for these layer counts, num_stack and n_components";
    if (o->num_tensors != gd::bc_num_tensors(o->fusion_layers, o->branch_layers, o->head_layers))
        return "num_tensors is not the state dict's tensor count for these layer counts";
    if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0)) return "betas must be in [0, 1)";
    if (!(o->eps > 0.f) || !(o->max_grad_norm > 0.f)) return "eps and max_grad_norm must be positive";
    if (!(o->weight_decay >= 0.f) || !std::isfinite(o->weight_decay)) return "weight_decay must be finite and not negative";
    if (!o->tensor_end || !o->lr || !o->step || !o->beta_pow || !o->params || !o->exp_avg || !o->exp_avg_sq || !o->blob ||
        !o->blob_of || !o->stats || !o->stats_sum || !o->max_grad_tensor || !o->tensor_norms || !o->scal)
        return "tensor_end, lr, step, beta_pow, params, exp_avg, exp_avg_sq, blob, blob_of, stats, stats_sum, max_grad_tensor, "
               "tensor_norms and scal are required";
    if (misaligned(o->beta_pow, 8) || misaligned(o->scal, 8) || misaligned(grad, 4) || misaligned(o->tensor_end, 4) ||
        misaligned(o->lr, 4) || misaligned(o->step, 4) || misaligned(o->params, 4) || misaligned(o->exp_avg, 4) ||
        misaligned(o->exp_avg_sq, 4) || misaligned(o->blob, 4) || misaligned(o->blob_of, 4) || misaligned(o->stats, 4) ||
        misaligned(o->stats_sum, 4) || misaligned(o->max_grad_tensor, 4) || misaligned(o->tensor_norms, 4))
        return "beta_pow and scal must be 8-byte aligned, the other buffers 4-byte aligned";
    return nullptr;
}

// The one checked optimiser step behind gd_bc_adamw and gd_bc_adamw_dim.  The order of refusal: the width, then opt and grad at
// that width.  The kernels have no width in them; it only sizes the two layouts opt must describe.
static int bc_adamw(const char *who, const gd_bc_opt *opt, int dim, const float *grad, void *stream) {
    const char *why = dim != 64 && dim != 128 ? "network_dim must be 64 or 128" : nullptr;
    if (!why) why = bc_adamw_problem(opt, grad, dim);
    if (why) return fail(GD_ERR_INVALID, std::string(who) + ": " + why);
    return guarded([&]() {
        gd::launch_bc_adamw(*opt, static_cast<hipStream_t>(stream), grad);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_bc_adamw(const gd_bc_opt *opt, const float *grad, void *stream) { return bc_adamw("gd_bc_adamw", opt, 64, grad, stream); }

int gd_bc_adamw_dim(const gd_bc_opt *opt, int32_t network_dim, const float *grad, void *stream) {
    return bc_adamw("gd_bc_adamw_dim", opt, network_dim, grad, stream);
}

// The one checked gradient step behind gd_bc_update and gd_bc_update_dim.  The order of refusal: the _dim struct, a NULL struct,
// then the forward, the row statistics, the backward and the optimiser step in the order they run, each sized at the width,
// then what ties the three structs together.
static int bc_update(const char *who, BCAt at, const gd_bc_grad *g, const gd_bc_opt *opt, const float *obs,
                     const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n, const float *expert_actions, void *stream) {
    if (at.why) return fail(GD_ERR_INVALID, std::string(who) + ": " + at.why);
    const gd_bc_policy *p = at.p;
    if (!p || !g || !opt) return fail(GD_ERR_INVALID, std::string(who) + ": null argument");
    const gd_bc_opt &o = *opt;
    gd_bc_outputs out{};
    out.actions = o.actions, out.nll = o.nll;
    const char *why = nullptr;
    if (!expert_actions || !o.actions || !o.nll || !o.grad_nll || !o.grad)
        why = "null argument (expert_actions, or opt's actions, nll, grad_nll or grad)";
    if (!why) why = bc_forward_problem(p, obs, partner_mask, road_mask, n, 1, nullptr, nullptr, expert_actions, &out, at.dim);
    if (!why) why = bc_train_rows_problem(opt, n, o.nll, o.actions, expert_actions, o.grad_nll);
    if (!why) why = bc_backward_problem(p, g, obs, partner_mask, road_mask, n, expert_actions, o.grad_nll, nullptr, o.grad, at.dim);
    if (!why) why = bc_adamw_problem(opt, o.grad, at.dim);
    if (!why && (o.max_rows < 1 || o.max_rows > (1 << 20))) why = "max_rows must be in [1, 2^20]";
    if (!why && n > o.max_rows) why = "n is above max_rows (the row scratch holds max_rows rows)";
    if (!why && (p->num_stack != o.num_stack || p->fusion_layers != o.fusion_layers || p->branch_layers != o.branch_layers ||
                 p->head_layers != o.head_layers || p->n_components != o.n_components || p->blob_floats != o.blob_floats ||
                 g->grad_floats != o.grad_floats))
        why = "the configurations and sizes of the policy, the backward and opt differ";
    if (!why && p->blob != o.blob) why = "the policy's blob must be opt's (the optimiser step updates it in place)";
    if (why) return fail(GD_ERR_INVALID, std::string(who) + ": " + why);
    return guarded([&]() {
        hipStream_t st = static_cast<hipStream_t>(stream);
        gd::launch_bc_forward(*p, at.dim, st, obs, partner_mask, road_mask, n, true, nullptr, nullptr, expert_actions, out);
        gd::launch_bc_train_rows(o, st, n, o.nll, o.actions, expert_actions, o.grad_nll);
        gd::launch_bc_backward(*p, at.dim, *g, st, obs, partner_mask, road_mask, n, expert_actions, o.grad_nll, nullptr, o.grad);
        gd::launch_bc_adamw(o, st, o.grad);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_bc_update(const gd_bc_policy *p, const gd_bc_grad *g, const gd_bc_opt *opt, const float *obs, const uint8_t *partner_mask,
                 const uint8_t *road_mask, int32_t n, const float *expert_actions, void *stream) {
    return bc_update("gd_bc_update", bc_at(p), g, opt, obs, partner_mask, road_mask, n, expert_actions, stream);
}

int gd_bc_update_dim(const gd_bc_policy_dim *p, const gd_bc_grad *g, const gd_bc_opt *opt, const float *obs,
                     const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n, const float *expert_actions, void *stream) {
    return bc_update("gd_bc_update_dim", bc_at(p), g, opt, obs, partner_mask, road_mask, n, expert_actions, stream);
}

int gd_bc_eval_accumulate(int32_t n, const float *nll, const float *actions, const float *expert_actions, float *acc, void *stream) {
    if (!nll || !actions || !expert_actions || !acc) return fail(GD_ERR_INVALID, "gd_bc_eval_accumulate: null argument");
    if (n < 1 || n > (1 << 20)) return fail(GD_ERR_INVALID, "gd_bc_eval_accumulate: n must be in [1, 2^20]");
    if (misaligned(nll, 4) || misaligned(actions, 4) || misaligned(expert_actions, 4) || misaligned(acc, 4))
        return fail(GD_ERR_INVALID, "gd_bc_eval_accumulate: float buffers must be 4-byte aligned");
    return guarded([&]() {
        gd::launch_bc_eval_accumulate(static_cast<hipStream_t>(stream), n, nll, actions, expert_actions, acc);
        HIP_CHECK(hipGetLastError());
    });
}

// The body of gd_bc_hidden (layer == nullptr: the tapped block's last layer) and gd_bc_hidden_layer.  The tokens are 64 wide.
static int bc_hidden(const char *who, const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                     int32_t n, int32_t tap, const int32_t *layer, float *out, void *stream) {
    gd_bc_outputs none{};
    const char *why = bc_forward_problem(p, obs, partner_mask, road_mask, n, 1, nullptr, nullptr, nullptr, &none, 64);
    if (!why && tap != GD_LP_TAP_FUSION && tap != GD_LP_TAP_RO) why = "tap must be GD_LP_TAP_FUSION or GD_LP_TAP_RO";
    if (!why && layer && (*layer < 0 || *layer >= (tap == GD_LP_TAP_RO ? p->branch_layers : p->fusion_layers)))
        why = "layer must be in [0, layers of the tapped block)";
    if (!why && (!out || misaligned(out, 16))) why = "out is required, 16-byte aligned";
    if (why) return fail(GD_ERR_INVALID, std::string(who) + ": " + why);
    return guarded([&]() {
        gd::launch_bc_hidden(*p, static_cast<hipStream_t>(stream), obs, partner_mask, road_mask, n, tap, out, layer ? *layer : -1);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_bc_hidden(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n, int32_t tap,
                 float *out, void *stream) {
    return bc_hidden("gd_bc_hidden", p, obs, partner_mask, road_mask, n, tap, nullptr, out, stream);
}

int gd_bc_hidden_layer(const gd_bc_policy *p, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask, int32_t n,
                       int32_t tap, int32_t layer, float *out, void *stream) {
    return bc_hidden("gd_bc_hidden_layer", p, obs, partner_mask, road_mask, n, tap, &layer, out, stream);
}

// everything the three gd_lp_* entries refuse; nullptr when everything is in order.  mode: launch_lp's
static const char *lp_problem(const gd_bc_policy *p, const gd_lp_probe *lp, const float *obs, const uint8_t *partner_mask,
                              const uint8_t *road_mask, int32_t n, const uint8_t *mask, const int64_t *labels, const gd_lp_rows *rows,
                              int mode, const int32_t *acc) {
    if (!lp || !obs) return "null argument";
    if (lp->model < GD_LP_EARLY || lp->model > GD_LP_BASELINE) return "model must be GD_LP_EARLY, GD_LP_LATE or GD_LP_BASELINE";
    if (lp->exp != GD_IL_FUTURE_OTHER && lp->exp != GD_IL_FUTURE_EGO) return "exp must be GD_IL_FUTURE_OTHER or GD_IL_FUTURE_EGO";
    if (lp->reserved[0] != 0 || lp->reserved[1] != 0) return "reserved must be 0";
    if (lp->max_agents != 64 && lp->max_agents != 128) return "max_agents must be 64 or 128";
    if (lp->num_stack < 1 || lp->num_stack > 8) return "num_stack must be in [1, 8]";
    if (lp->model == GD_LP_BASELINE) {
        if (p) return "the baseline probe takes no policy";
        if (n < 1 || n > (1 << 20)) return "n must be in [1, 2^20]";
        if (misaligned(obs, 4)) return "float and int32 buffers must be 4-byte aligned";
        const int k = (lp->exp == GD_IL_FUTURE_OTHER ? 12 : 6) * lp->num_stack;
        if (k > 64) return "the baseline probe's in_features (12 num_stack for 'other') must not exceed 64";
        if (lp->in_features != k) return "in_features must be 6 num_stack ('ego') or 12 num_stack ('other') for the baseline probe";
    } else {
        gd_bc_outputs none{};
        if (const char *why = bc_forward_problem(p, obs, partner_mask, road_mask, n, 1, nullptr, nullptr, nullptr, &none, 64)) return why;
        if (lp->max_agents != p->max_agents || lp->num_stack != p->num_stack) return "max_agents and num_stack must be the policy's";
        if (lp->in_features != 64) return "in_features must be 64 with a policy";
    }
    if (lp->num_partials < 1 || lp->num_partials > 4096) return "num_partials must be in [1, 4096]";
    if (!lp->packed || misaligned(lp->packed, 16)) return "packed is required, 16-byte aligned";
    if (rows && (misaligned(rows->logits, 16) || misaligned(rows->loss_row, 4) || misaligned(rows->pred, 8)))
        return "logits must be 16-byte aligned, loss_row 4-byte, pred 8-byte";
    if (mode == 0) {
        if (!rows || (!rows->logits && !rows->pred)) return "rows with logits or pred is required";
        if (rows->loss_row) return "loss_row needs labels (gd_lp_update, gd_lp_eval_accumulate)";
        return nullptr;
    }
    if (!mask || !labels || misaligned(labels, 8)) return "mask and labels are required, labels 8-byte aligned";
    if (!lp->part_f || !lp->part_d || !lp->part_i || misaligned(lp->part_f, 4) || misaligned(lp->part_d, 8) || misaligned(lp->part_i, 4))
        return "part_f, part_d and part_i are required (4-, 8- and 4-byte aligned)";
    if (misaligned(lp->stats, 4)) return "float and int32 buffers must be 4-byte aligned";
    if (mode == 2) return !acc || misaligned(acc, 8) ? "acc is required, 8-byte aligned" : nullptr;
    if (!(lp->beta1 >= 0.0 && lp->beta1 < 1.0) || !(lp->beta2 >= 0.0 && lp->beta2 < 1.0)) return "betas must be in [0, 1)";
    if (!(lp->eps > 0.f)) return "eps must be positive";
    if (!(lp->weight_decay >= 0.f) || !std::isfinite(lp->weight_decay)) return "weight_decay must be finite and not negative";
    if (!lp->weight || !lp->exp_avg || !lp->exp_avg_sq || !lp->lr || !lp->step || !lp->beta_pow || !lp->grad || !lp->stats || !lp->sums ||
        !lp->counts || !lp->scal)
        return "weight, exp_avg, exp_avg_sq, lr, step, beta_pow, grad, stats, sums, counts and scal are required";
    if (misaligned(lp->beta_pow, 8) || misaligned(lp->sums, 8) || misaligned(lp->weight, 4) || misaligned(lp->exp_avg, 4) ||
        misaligned(lp->exp_avg_sq, 4) || misaligned(lp->lr, 4) || misaligned(lp->step, 4) || misaligned(lp->grad, 4) ||
        misaligned(lp->counts, 4) || misaligned(lp->scal, 4))
        return "beta_pow and sums must be 8-byte aligned, the other buffers 4-byte aligned";
    return nullptr;
}

int gd_lp_forward(const gd_bc_policy *p, const gd_lp_probe *lp, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                  int32_t n, const gd_lp_rows *rows, void *stream) {
    if (const char *why = lp_problem(p, lp, obs, partner_mask, road_mask, n, nullptr, nullptr, rows, 0, nullptr))
        return fail(GD_ERR_INVALID, std::string("gd_lp_forward: ") + why);
    return guarded([&]() {
        gd::launch_lp(p, *lp, static_cast<hipStream_t>(stream), obs, partner_mask, road_mask, n, nullptr, nullptr, rows, 0, nullptr);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_lp_update(const gd_bc_policy *p, const gd_lp_probe *lp, const float *obs, const uint8_t *partner_mask, const uint8_t *road_mask,
                 int32_t n, const uint8_t *mask, const int64_t *labels, const gd_lp_rows *rows, void *stream) {
    if (const char *why = lp_problem(p, lp, obs, partner_mask, road_mask, n, mask, labels, rows, 1, nullptr))
        return fail(GD_ERR_INVALID, std::string("gd_lp_update: ") + why);
    return guarded([&]() {
        gd::launch_lp(p, *lp, static_cast<hipStream_t>(stream), obs, partner_mask, road_mask, n, mask, labels, rows, 1, nullptr);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_lp_eval_accumulate(const gd_bc_policy *p, const gd_lp_probe *lp, const float *obs, const uint8_t *partner_mask,
                          const uint8_t *road_mask, int32_t n, const uint8_t *mask, const int64_t *labels, const gd_lp_rows *rows,
                          int32_t *acc, void *stream) {
    if (const char *why = lp_problem(p, lp, obs, partner_mask, road_mask, n, mask, labels, rows, 2, acc))
        return fail(GD_ERR_INVALID, std::string("gd_lp_eval_accumulate: ") + why);
    return guarded([&]() {
        gd::launch_lp(p, *lp, static_cast<hipStream_t>(stream), obs, partner_mask, road_mask, n, mask, labels, rows, 2, acc);
        HIP_CHECK(hipGetLastError());
    });
}

int gd_episode_step(gd_sim *s, const gd_episode_config *cfg, const gd_episode_buffers *b) {
    if (!s || !cfg || !b) return fail(GD_ERR_INVALID, "gd_episode_step: null argument");
    if (!b->controlled_mask || !b->agent_episode_returns || !b->episode_lengths || !b->collided_in_episode ||
        !b->offroad_in_episode || !b->live_agent_mask || !b->reward_out || !b->terminal_out || !b->truncated_out ||
        !b->mask_out || !b->done_worlds || !b->stats || !b->world_stats)
        return fail(GD_ERR_INVALID, "gd_episode_step: every buffer is required");
    if (cfg->reward_type < GD_EPISODE_REWARD_WEIGHTED || cfg->reward_type > GD_EPISODE_REWARD_LOG_DISTANCE)
        return fail(GD_ERR_INVALID, "gd_episode_step: unknown reward_type");
    if (cfg->reward_type == GD_EPISODE_REWARD_CONDITIONED && (!b->reward_weights || !b->weight_draws))
        return fail(GD_ERR_INVALID, "gd_episode_step: reward_conditioned needs reward_weights and weight_draws");
    if (cfg->reward_type == GD_EPISODE_REWARD_CONDITIONED &&
        (cfg->condition_mode < GD_CONDITION_RANDOM || cfg->condition_mode > GD_CONDITION_FIXED))
        return fail(GD_ERR_INVALID, "gd_episode_step: unknown condition_mode");
    if ((b->reward_rows || b->terminal_rows || b->truncated_rows || b->mask_rows) && !s->d.row_of_slot)
        return fail(GD_ERR_INVALID, "gd_episode_step: flat outputs need learner rows (gd_set_learner_rows)");
    return guarded([&]() {
        HIP_CHECK(hipMemsetAsync(s->d.any_reset, 0, sizeof(int32_t), s->stream));
        gd::launch_episode_step(s->d, s->stream, *cfg, *b);
        HIP_CHECK(hipGetLastError());
        if (cfg->auto_reset) s->reset_flagged(true);
    });
}

int gd_episode_set_warmup(gd_sim *s, int32_t init_steps, int32_t scope) {
    if (init_steps < 0 || init_steps >= GD_EPISODE_LEN)
        return fail(GD_ERR_INVALID, "gd_episode_set_warmup: init_steps must be in [0, 90] (the expert trajectory has 91 steps)");
    if (scope != GD_WARMUP_RESET_WORLDS && scope != GD_WARMUP_ALL_WORLDS)
        return fail(GD_ERR_INVALID, "gd_episode_set_warmup: unknown scope (GD_WARMUP_RESET_WORLDS or GD_WARMUP_ALL_WORLDS)");
    if (!s) return fail(GD_ERR_INVALID, "gd_episode_set_warmup: null sim");
    // Only the gated reset pass reads these fields; the captured step graph holds step passes, which never do, so it stays.
    s->d.warm_k = init_steps;
    s->d.warm_all = scope == GD_WARMUP_ALL_WORLDS ? 1 : 0;
    return GD_OK;
}

int gd_episode_draw_weights(gd_sim *s, const gd_episode_config *cfg, const gd_episode_buffers *b, const int32_t *worlds,
                            int32_t n) {
    if (!s || !cfg || !b || !b->reward_weights || !b->weight_draws || (worlds && n < 0))
        return fail(GD_ERR_INVALID, "gd_episode_draw_weights: bad argument");
    if (cfg->condition_mode < GD_CONDITION_RANDOM || cfg->condition_mode > GD_CONDITION_FIXED)
        return fail(GD_ERR_INVALID, "gd_episode_draw_weights: unknown condition_mode");
    std::vector<int32_t> list;
    if (worlds) {
        list.assign(worlds, worlds + n);
        for (const int32_t w : list)
            if (w < 0 || w >= s->W) return fail(GD_ERR_INVALID, "gd_episode_draw_weights: world index out of range");
        std::sort(list.begin(), list.end());  // a world listed twice is drawn once (one workgroup per world)
        list.erase(std::unique(list.begin(), list.end()), list.end());
        if (list.empty()) return GD_OK;
    }
    return guarded([&]() {
        if (!worlds) {
            gd::launch_draw_weights(s->d, s->stream, *cfg, *b, nullptr, s->W);
            HIP_CHECK(hipGetLastError());
            return;
        }
        // an explicit call outside the step path: a temporary device copy of the list, waited for before it is freed
        const gd::DevMem dl(list.size() * sizeof(int32_t));
        hipError_t e = hipMemcpyAsync(dl.get(), list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, s->stream);
        if (e == hipSuccess) {
            gd::launch_draw_weights(s->d, s->stream, *cfg, *b, static_cast<const int32_t *>(dl.get()), static_cast<int>(list.size()));
            e = hipGetLastError();
        }
        const hipError_t es = hipStreamSynchronize(s->stream);  // before dl goes, whatever failed
        HIP_CHECK(e);
        HIP_CHECK(es);
    });
}

int gd_sync(gd_sim *s) {
    if (!s) return fail(GD_ERR_INVALID, "gd_sync: null sim");
    return guarded([&]() { HIP_CHECK(hipStreamSynchronize(s->stream)); });
}

int gd_set_stream(gd_sim *s, void *stream) {
    if (!s) return fail(GD_ERR_INVALID, "gd_set_stream: null sim");
    return guarded([&]() {
        HIP_CHECK(hipStreamSynchronize(s->stream));
        s->drop_graph();
        HIP_CHECK(hipStreamSynchronize(s->side.get()));
        s->stream = static_cast<hipStream_t>(stream);
        s->d.split_partner = (s->stream != nullptr && std::getenv("GPUDRIVE_SPLIT_PARTNER") != nullptr) ? 1 : 0;
    });
}

int gd_attach_bev(gd_sim *s, float *bev) {
    if (!s || !bev) return fail(GD_ERR_INVALID, "gd_attach_bev: null argument");
    return guarded([&]() {
        if (s->d.bev && s->d.bev != bev) throw std::runtime_error("gd_attach_bev: a BEV tensor is already attached");
        HIP_CHECK(hipStreamSynchronize(s->stream));
        s->drop_graph();
        s->exported[GD_T_BEV] = bev;
        s->d.bev = bev;
        HIP_CHECK(hipMemsetAsync(s->d.bev_dirty, 1, sizeof(int32_t) * static_cast<size_t>(s->W) * s->A, s->stream));
        if (!s->params.disableClassicalObs) s->launch(gd::KERNEL_BEV, false);  // the rasters of the current state
    });
}

int gd_stat(gd_sim *s, int32_t which, int64_t *out) {
#ifdef GD_CLOCKS
    if (s && out && which >= 22 && which <= 29) {  // the set-order selection's phase clocks (map_obs.hip g_set_clk): 22 reads and zeroes all
        static unsigned long long clk[8];
        if (which == 22) gd::set_clocks_read(clk);
        *out = (int64_t)clk[which - 22];
        return GD_OK;
    }
#endif
#ifdef GD_CLOCKS
    if (s && out && which >= 32 && which <= 43) {  // k_world_step's phase clocks and counters (kernels.hip g_step_clk / g_step_cnt): 32 reads and zeroes all
        static unsigned long long clk[12];
        if (which == 32) gd::step_clocks_read(clk);
        *out = (int64_t)clk[which - 32];
        return GD_OK;
    }
#endif
#ifdef GD_CLOCKS
    if (s && out && which >= 1000 && which < 1256) {  // k_knn_replay's phase clocks of the last selection (map_obs_rank.hip ReplayClock): rk_hist[256 + k]
        *out = 0;
        if (s->rk_alloc) {
            int32_t v = 0;
            (void)hipStreamSynchronize(s->stream);
            if (hipMemcpy(&v, s->d.rk_hist + 256 + (which - 1000), sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(GD_ERR_DEVICE, "gd_stat: reading the replay clocks failed");
            *out = v;
        }
        return GD_OK;
    }
#endif
#ifdef GD_WAVE_CLOCKS
    if (s && out && which >= 2000 && which < 2000 + 3 * GD_RANK_GRID) {  // k_knn_rank's waves in the last selection (engine.hpp GD_RH_WAVES)
        *out = 0;
        if (s->rk_alloc) {
            int32_t v = 0;
            (void)hipStreamSynchronize(s->stream);
            if (hipMemcpy(&v, s->d.rk_hist + GD_RH_WAVES + (which - 2000), sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(GD_ERR_DEVICE, "gd_stat: reading the ranking waves' clocks failed");
            *out = v;
        }
        return GD_OK;
    }
#endif
#if defined(GD_DIAG) || defined(GD_CLOCKS)
    constexpr int32_t kLastStat = 20;
#else
    constexpr int32_t kLastStat = 7;
#endif
    if (s && out && which == 30) {  // agents whose road rows were left in place (pose unchanged) since the last read
        std::vector<unsigned long long> v(GD_SKIP_SLOTS, 0);
        (void)hipStreamSynchronize(s->stream);
        if (hipMemcpy(v.data(), s->d.stat_skipped, sizeof(unsigned long long) * v.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemset(s->d.stat_skipped, 0, sizeof(unsigned long long) * v.size()) != hipSuccess)
            return fail(GD_ERR_DEVICE, "gd_stat: reading the skip counters failed");
        unsigned long long sum = 0;
        for (unsigned long long x : v) sum += x;
        *out = static_cast<int64_t>(sum) + s->host_skipped;
        s->host_skipped = 0;
        return GD_OK;
    }
    if (s && out && which == 31) {  // BEV rasters painted by the last pass that rasterised (bev_lidar.hip k_bev_list's count)
        int32_t c = 0;
        (void)hipStreamSynchronize(s->stream);
        if (hipMemcpy(&c, s->d.bev_count, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(GD_ERR_DEVICE, "gd_stat: reading the raster count failed");
        *out = c;
        return GD_OK;
    }
    if (s && out && which == 44) {  // agents whose LiDAR returns the last pass marked for tracing (the others were left in place)
        std::vector<int32_t> f(static_cast<size_t>(s->W) * s->A), n(static_cast<size_t>(s->W) * 2);
        (void)hipStreamSynchronize(s->stream);
        if (hipMemcpy(f.data(), s->d.lidar_dirty, sizeof(int32_t) * f.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(n.data(), s->d.shape, sizeof(int32_t) * n.size(), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(GD_ERR_DEVICE, "gd_stat: reading the LiDAR flags failed");
        int64_t c = 0;
        for (int w = 0; w < s->W; w++)
            for (int a = 0; a < n[static_cast<size_t>(w) * 2] && a < s->A; a++) c += f[static_cast<size_t>(w) * s->A + a] != 0;
        *out = c;
        return GD_OK;
    }
    if (s && out && which == 45) {  // indices outside the table that gd_set_discrete_actions met, since the sim was created
        unsigned long long v = 0;
        (void)hipStreamSynchronize(s->stream);
        if (hipMemcpy(&v, s->d.bad_actions, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(GD_ERR_DEVICE, "gd_stat: reading the action counter failed");
        *out = static_cast<int64_t>(v);
        return GD_OK;
    }
    if (s && out && which == 46) {  // worlds the warm-up of the device auto-reset advanced, since the sim was created
        unsigned long long v = 0;
        (void)hipStreamSynchronize(s->stream);
        if (hipMemcpy(&v, s->d.warm_count, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(GD_ERR_DEVICE, "gd_stat: reading the warm-up counter failed");
        *out = static_cast<int64_t>(v);
        return GD_OK;
    }
    if (s && out && which == 47) {  // 1: the state step runs the set-up of the rank path itself (engine.hpp rank_setup_folded)
        *out = gd::rank_setup_folded(s->d) ? 1 : 0;
        return GD_OK;
    }
    if (s && out && which == 22) {  // checkpoint rows k_knn_scan wrote in the last selection (engine.hpp GD_RH_ROWS)
        *out = 0;
        if (s->rk_alloc) {
            int32_t v = 0;
            (void)hipStreamSynchronize(s->stream);
            if (hipMemcpy(&v, s->d.rk_hist + GD_RH_ROWS, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(GD_ERR_DEVICE, "gd_stat: reading the row counter failed");
            *out = v;
        }
        return GD_OK;
    }
    if (s && out && which == 21) {  // bounds audit of the rank path (engine.hpp GD_RANK_AUDIT): violations since the buffers exist
        *out = 0;
        if (s->rk_alloc) {
            int32_t v = 0;
            (void)hipStreamSynchronize(s->stream);
            if (hipMemcpy(&v, s->d.rk_hist + GD_RANK_AUDIT, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(GD_ERR_DEVICE, "gd_stat: reading the audit counter failed");
            *out = v;
        }
        return GD_OK;
    }
    if (!s || !out || which < 0 || which > kLastStat) return fail(GD_ERR_INVALID, "gd_stat: bad argument");
#if defined(GD_DIAG) || defined(GD_CLOCKS)
    if (which >= 8) {  // 8 = most crowded ranking bucket (-DGD_DIAG, GPUDRIVE_RANK_DBG=9), 10..17 = clock ticks / 256 per phase of
                       // k_knn_rank summed over its waves, 18..20 = k_knn_replay's rounds of its first wave / candidates beyond K /
                       // inserts (-DGD_CLOCKS); since the last read
        *out = 0;
        if (s->rk_alloc) {
            int32_t v = 0;
            (void)hipStreamSynchronize(s->stream);
            (void)hipMemcpy(&v, s->d.rk_hist + 514 + (which - 8), sizeof(v), hipMemcpyDeviceToHost);
            (void)hipMemset(s->d.rk_hist + 514 + (which - 8), 0, sizeof(v));
            *out = v;
        }
        return GD_OK;
    }
#endif
    if (which == 7) {  // 1: the reference-order road selection takes the rank replay (map_obs_rank.hip)
        *out = s->d.rk_on;
        return GD_OK;
    }
    *out = which == 0 ? s->stat_graph_steps : which == 1 ? s->stat_plain_steps : which == 2 ? s->stat_captures
         : which == 3 ? s->d.set_fused_rows : which == 4 ? s->d.set_apw : which == 5 ? s->d.live_count : GD_MAP_OBS_AW;
    return GD_OK;
}

int gd_kernel_timing_enable(gd_sim *s, int32_t enable) {
    if (!s) return fail(GD_ERR_INVALID, "null sim");
    return guarded([&]() {
        HIP_CHECK(hipStreamSynchronize(s->stream));
        for (int k = 0; k < gd::KERNEL_TIMED; k++) {
            s->collect_timing(k);
            s->ev_ms[k] = 0;
            s->ev_launches[k] = 0;
            while (enable && s->ev_pool[k].size() < gd_sim::kEvRing) {  // every event exists before the first timed launch
                s->ev_pool[k].push_back(EventPair{make_event(), make_event()});  // (a failing second one returns the first)
            }
        }
        s->timing = enable != 0;
    });
}

int gd_kernel_timing_read(gd_sim *s, int32_t kernel, double *total_ms, int64_t *launches) {
    if (!s || kernel < 0 || kernel >= gd::KERNEL_TIMED) return fail(GD_ERR_INVALID, "gd_kernel_timing_read: bad argument");
    return guarded([&]() {
        HIP_CHECK(hipStreamSynchronize(s->stream));
        s->collect_timing(kernel);
        if (total_ms) *total_ms = s->ev_ms[kernel];
        if (launches) *launches = s->ev_launches[kernel];
    });
}

int gd_debug_get_state(gd_sim *s, float *out) {
    if (!s || !out) return fail(GD_ERR_INVALID, "null argument");
    return guarded([&]() {
        HIP_CHECK(hipStreamSynchronize(s->stream));
        const size_t WA = static_cast<size_t>(s->W) * s->A;
        std::vector<float> plane(WA);
        std::vector<int32_t> iplane(WA);
        const float *src[8] = {s->d.px, s->d.py, s->d.pz, s->d.qw, s->d.qz, s->d.vx, s->d.vy, s->d.vz};
        const int dstcol[8] = {0, 1, 2, 3, 6, 7, 8, 9};
        for (size_t i = 0; i < WA * 11; i++) out[i] = 0.f;
        for (int k = 0; k < 8; k++) {
            HIP_CHECK(hipMemcpy(plane.data(), src[k], WA * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < WA; i++) out[i * 11 + dstcol[k]] = plane[i];
        }
        for (size_t i = 0; i < WA; i++) {  // x, y = 0 * z as produced by angleAxis
            out[i * 11 + 4] = 0.f * out[i * 11 + 6];
            out[i * 11 + 5] = 0.f * out[i * 11 + 6];
        }
        HIP_CHECK(hipMemcpy(iplane.data(), s->d.collided, WA * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < WA; i++) out[i * 11 + 10] = static_cast<float>(iplane[i]);
    });
}

int gd_debug_road_path(gd_sim *s, int32_t *out) {
    if (!s || !out) return fail(GD_ERR_INVALID, "null argument");
    return guarded([&]() {
        HIP_CHECK(hipStreamSynchronize(s->stream));
        const size_t WA = static_cast<size_t>(s->W) * s->A;
        if (!s->rk_alloc || !s->d.rk_on) {
            for (size_t i = 0; i < WA; i++) out[i] = -2;
            return;
        }
        HIP_CHECK(hipMemcpy(out, s->d.rk_n, WA * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<int32_t> why(WA);
        HIP_CHECK(hipMemcpy(why.data(), s->d.rk_ticket, WA * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < WA; i++) {
            if (out[i] > 0) out[i] = out[i] == (1 << 30) ? -3 : (out[i] & 0xffff);
            else if (out[i] == -1 && why[i] < -1) out[i] = -10 + (why[i] + 2);  // -10 no checkpoints / small world, -11 overflow, -13 bypass
            else if (out[i] == -1 && why[i] >= 0 && ((why[i] >> 30) & 1)) out[i] = -12;  // more than 32 candidates with one key
        }
    });
}

int gd_debug_set_state(gd_sim *s, const float *in) {
    if (!s || !in) return fail(GD_ERR_INVALID, "null argument");
    return guarded([&]() {
        HIP_CHECK(hipStreamSynchronize(s->stream));
        const size_t WA = static_cast<size_t>(s->W) * s->A;
        std::vector<float> plane(WA);
        std::vector<int32_t> iplane(WA);
        float *dst[8] = {s->d.px, s->d.py, s->d.pz, s->d.qw, s->d.qz, s->d.vx, s->d.vy, s->d.vz};
        const int srccol[8] = {0, 1, 2, 3, 6, 7, 8, 9};
        for (int k = 0; k < 8; k++) {
            for (size_t i = 0; i < WA; i++) plane[i] = in[i * 11 + srccol[k]];
            HIP_CHECK(hipMemcpy(dst[k], plane.data(), WA * 4, hipMemcpyHostToDevice));
        }
        for (size_t i = 0; i < WA; i++) iplane[i] = in[i * 11 + 10] != 0.f;
        HIP_CHECK(hipMemcpy(s->d.collided, iplane.data(), WA * 4, hipMemcpyHostToDevice));
        // agents that never move are not on the linear scan's step-pass list: the next road pass must visit them all the same
        // ... and k_world_step's "who moved" (the BEV's dirty flags) compares the poses before and after its own movement only
        s->full_pass_next = (s->params.roadObservationAlgorithm != GD_ROADS_K_NEAREST && s->d.lin_on != 0) || s->d.bev != nullptr ||
                            (s->d.lidar != nullptr && s->params.enableLidar);
    });
}

int gd_host_world_build(const char *scene, const gd_params *params, int32_t A, const int32_t *deleted, int32_t ndel,
                        gd_host_world *out) {
    if (!scene || !params || !out || A < 2 || A > GD_MAX_AGENTS_LIMIT) return fail(GD_ERR_INVALID, "gd_host_world_build: bad argument");
    std::memset(out, 0, sizeof(*out));
    return guarded([&]() {
        auto map = gd::load_scene(scene, params->polylineReductionThreshold);
        gd::HostWorld hw;
        gd::build_host_world(*map, *params, A, deleted, ndel, hw);
        out->num_agents = hw.num_agents;
        out->num_roads = hw.num_roads;
        out->num_collidable_roads = static_cast<int32_t>(hw.boxes.size());
        out->max_agents = A;
        std::memcpy(out->mean, hw.mean, sizeof(hw.mean));
        std::memcpy(out->map_name, hw.map_name, sizeof(hw.map_name));
        std::memcpy(out->scenario_id, hw.scenario_id, sizeof(hw.scenario_id));
        auto dupf = [](const std::vector<float> &v, size_t n) {
            float *p = static_cast<float *>(std::calloc(std::max<size_t>(n, 1), sizeof(float)));
            std::memcpy(p, v.data(), std::min(n, v.size()) * sizeof(float));
            return p;
        };
        auto dupi = [](const std::vector<int32_t> &v) {
            int32_t *p = static_cast<int32_t *>(std::calloc(std::max<size_t>(v.size(), 1), sizeof(int32_t)));
            std::memcpy(p, v.data(), v.size() * sizeof(int32_t));
            return p;
        };
        out->map_obs = dupf(hw.map_obs, static_cast<size_t>(GD_MAX_ROAD_ENTITIES) * 9);
        for (int r = hw.num_roads; r < GD_MAX_ROAD_ENTITIES; r++) { out->map_obs[r * 9 + 7] = -1.f; out->map_obs[r * 9 + 8] = -1.f; }
        out->trajectory = dupf(hw.trajectory, hw.trajectory.size());
        out->vehicle_size = dupf(hw.size, hw.size.size());
        out->goal = dupf(hw.goal, hw.goal.size());
        out->controlled = dupi(hw.controlled);
        out->response_type = dupi(hw.resp);
        out->agent_id = dupi(hw.agent_id);
        out->entity_type = dupi(hw.etype);
        out->metadata = dupi(hw.metadata);
    });
}

int gd_scene_cache_write(const char *scene, float polyline_reduction_threshold, const char *out_path) {
    if (!scene || !out_path) return fail(GD_ERR_INVALID, "gd_scene_cache_write: null argument");
    if (!gd::is_scene_cache_path(out_path)) return fail(GD_ERR_INVALID, "gd_scene_cache_write: the cache path must end in .gdsm");
    return guarded([&]() {
        auto map = gd::load_scene(scene, polyline_reduction_threshold);
        gd::write_scene_cache(*map, polyline_reduction_threshold, out_path);
    });
}

void gd_host_world_free(gd_host_world *w) {
    if (!w) return;
    std::free(w->map_obs); std::free(w->trajectory); std::free(w->vehicle_size); std::free(w->goal);
    std::free(w->controlled); std::free(w->response_type); std::free(w->agent_id); std::free(w->entity_type);
    std::free(w->metadata);
    std::memset(w, 0, sizeof(*w));
}

}  // extern "C"
