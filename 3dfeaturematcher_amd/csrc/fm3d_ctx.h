// fm3d_ctx.h -- the context behind the C ABI's opaque fm3d_ctx, its self-freeing buffers and the few
// helpers that more than one translation unit of the library uses (private, like fm3d_internal.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "fm3d.h"
#include "fm3d_algebra.h"
#include "fm3d_kernels.h"

namespace fm3d_host {

// A block of memory that grows on demand and frees itself; move-only.  Mem names the allocator:
// DeviceMem (hipMalloc) or PinnedMem (hipHostMalloc).  ensure() grows only, and frees the old block
// before it allocates the new one.  hipFree and hipHostFree synchronise the device first, so a block
// that queued work still names outlives that work -- when ensure() grows as at scope exit.
//
// Test hook FM3D_DEBUG_POISON (tests/test_gpu_poison.py): when set, its value (strtoul, base 0) is a
// 32-bit word that fills every newly allocated block -- whole words and the tail bytes -- before
// ensure() returns, so a read of memory nothing wrote changes the result the same way every run.
// Read at each allocation; unset, it costs that one getenv.
inline bool poison_word(uint32_t* word) {
    const char* e = getenv("FM3D_DEBUG_POISON");
    if (!e || !e[0]) return false;
    *word = (uint32_t)strtoul(e, nullptr, 0);
    return true;
}
// the tail bytes continue the word's little-endian byte pattern
inline void poison_host(void* p, size_t n, uint32_t word) {
    uint8_t* b = (uint8_t*)p;
    for (size_t i = 0; i < n; i++) b[i] = (uint8_t)(word >> (8 * (i & 3)));
}
// A device block: filled on the null stream, then the device is synchronised -- the contexts'
// streams are non-blocking, so the null stream alone orders nothing before their work.
inline hipError_t poison_device(void* p, size_t n) {
    uint32_t word;
    if (!poison_word(&word)) return hipSuccess;
    hipError_t e = hipSuccess;
    if (n / 4) e = hipMemsetD32((hipDeviceptr_t)p, (int)word, n / 4);
    for (size_t i = n & ~(size_t)3; e == hipSuccess && i < n; i++)
        e = hipMemset((uint8_t*)p + i, (int)(uint8_t)(word >> (8 * (i & 3))), 1);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

template <class Mem>
struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            if (p) Mem::free(p);
            p = o.p;
            bytes = o.bytes;
            o.p = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~Buf() {
        if (p) Mem::free(p);
    }
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) Mem::free(p);
        p = nullptr;
        bytes = 0;
        size_t alloc = n < Mem::kMin ? Mem::kMin : n;
        hipError_t e = Mem::alloc(&p, alloc);
        if (e == hipSuccess) e = Mem::poison(p, alloc);
        if (e == hipSuccess) {
            bytes = alloc;
        } else if (p) {
            Mem::free(p);
            p = nullptr;
        }
        return e;
    }
    template <typename T>
    T* as() const {
        return (T*)p;
    }
};

struct DeviceMem {
    static constexpr size_t kMin = 256;
    static hipError_t alloc(void** p, size_t n) { return hipMalloc(p, n); }
    static hipError_t free(void* p) { return hipFree(p); }
    static hipError_t poison(void* p, size_t n) { return poison_device(p, n); }
};
// page-locked host staging: the H2D copies of the inputs run asynchronously from it, at full PCIe
// rate, and the host may return before they execute (fm3d_pipeline_submit)
struct PinnedMem {
    static constexpr size_t kMin = 4096;
    static hipError_t alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
    static hipError_t poison(void* p, size_t n) {  // on the host: nothing is queued on a new block
        uint32_t word;
        if (poison_word(&word)) poison_host(p, n, word);
        return hipSuccess;
    }
};
using DevBuf = Buf<DeviceMem>;
using HostBuf = Buf<PinnedMem>;

// (the LM gathers read a level's row-major bytes up to offset (h + 1) w + w + 1 < h w + kGuard(w))
constexpr size_t kGuard(int w) { return (size_t)4 * w + 64; }
// image 2's column-major level copies (LevelDesc::img2t): (w + 2) columns of stride kColStride(h),
// rows y >= h of every column and the bytes past the last column zero
constexpr int kColStride(int h) { return (h + 2 + 63) / 64 * 64; }
constexpr size_t kColBytes(int w, int h) { return (size_t)(w + 2) * kColStride(h) + 64; }

// the pipeline's small device -> host results of one frame pair (one D2H, pinned)
struct PipeSmall {
    int32_t cnt[4];                 // matches K, inliers P, kept, pad (c->pcnt bytes 0..15)
    unsigned long long prob[2];     // this pair's residual / pixel evaluations (c->pcnt bytes 16..31)
    unsigned long long lm[26];      // the LM launch's counters (fm3d_lm2.hip statPass layout)
};

// one direction's private buffers of a k = 2 search (knn2_search, fm3d_matching.cpp)
struct KnnWork {
    DevBuf cq, ct;            // u8: query constants, packed train constants
    DevBuf q8, t8;            // 256-bit rows unpacked: queries 0/1, train rows -1/+1
    DevBuf partIdx, partKey;  // per-part top-2 lists of the split matchers
    DevBuf pairs;             // float rows: the row-pair copy of the train side
    DevBuf idx, key, fkey;    // the merged top-2 lists
};

// The staged pair's state: what is queued on the context stream and not yet waited for.
//
//   state        entered by                                   left (to Idle) by
//   Idle         create; every wait; a run_* that returned    --
//   Full         submit (no leader), internal_enqueue;        wait, internal_finish
//                from MemberFront: the leader's next submit,
//                wait's or internal_flush's own LM
//   MemberFront  submit on a link member (front half only)    (to Full, see there)
//   DltFront     submit_dlt, submit_dlt_pair                  wait_dlt
//   Ncc          submit_ncc                                   wait_ncc
//   Verified     submit_verified                              wait_verified
//   DltVerified  submit_dlt_verified                          wait_dlt_verified
//
// Every other pipeline call needs Idle (most of them a staged pair too) and is refused otherwise; a
// submit that fails leaves Idle.  run_dlt and run_ncc are their submit followed by their wait.
// c->staged and c->specU8 describe the staged inputs, not the queue.  The one-shot calls
// (fm3d_knn2, fm3d_triangulate, fm3d_set_images, ...) do not look at the state: DESIGN.md §2.1.
enum class PairState { Idle, Full, MemberFront, DltFront, Ncc, Verified, DltVerified };

// what an entry point needs of the context before it does anything (require, fm3d_pipeline.cpp)
enum class Need { Idle, StagedIdle, Full, Dlt, Ncc, Verified, DltVerified };

// the timed events of a context, by what they mark on its stream
enum Ev {
    EV_LM_START,      // standalone fm3d_optimize_normals: before its launch
    EV_END,           // the end of whatever was queued last (standalone LM, every pipeline path)
    EV_FRONT_START,   // front half: before the match
    EV_MATCH_DONE,    // match + NNDR done (FM3D_STAGE_EVENTS)
    EV_DLT_DONE,      // triangulation done (FM3D_STAGE_EVENTS)
    EV_VERIFY_START, EV_VERIFY_END,  // the verified runs and submits: around the verification
    EV_NORMAL_START, EV_NORMAL_END,  // around the normal stage (LM or NCC scoring)
    EV_SUBMIT_START,  // a submit, before its inputs' H2D
    EV_TAIL_START,    // fm3d_pipeline_describe: before its first launch
    EV_COUNT
};

}  // namespace fm3d_host

using fm3d_host::DevBuf;
using fm3d_host::HostBuf;

struct fm3d_ctx {
    fm3d_settings s;
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    fm3d::Camera cam{};
    double g12[16];
    double R2[9], t2[3];
    bool haveG12 = false;
    // pyramids
    int w = 0, h = 0;
    std::vector<int> lw, lh;
    std::vector<DevBuf> pyr1, pyr2;
    std::vector<DevBuf> pyr2t;  // image 2's levels column-major (kColStride), for the LM gathers
    int lmCols = -1;            // the last LM launch's image-2 layout: 1 columns, 0 rows
    int pyrGuardW = -1, pyrGuardH = -1, pyrGuardLevels = -1;  // the geometry whose guards are zero
    DevBuf lvlDesc;
    // circle offsets of pixelsRay
    DevBuf offsets;
    int nOff = 0, nOffPad = 0;
    // work buffers
    DevBuf A, B, knnOut, cand, flag, matches, count, scanTmp;
    // the k = 2 searches' private buffers: forward, and the cross-check's reverse search (DESIGN.md
    // §3.1c; allocated only when it runs).  fwd.q8 / fwd.t8 are also the u8 rows packed from floats
    fm3d_host::KnnWork fwd, rev;
    DevBuf u8Flag;            // launch_f32_pack_u8's "not integer-valued" flag
    // the guided matchers' gate (fm3d_kernels.h EpiGate): query lines (float4) and train (u, v)
    DevBuf gLines, gUV;
    bool gateStaged = false;  // they belong to the staged pair's keypoints under the current g12
    bool specU8 = false;      // the staged float rows went to the u8 matcher before their flag was read
    // SURF detection / description
    DevBuf sfImg, sfSum, sfDet, sfTr, sfLayers, sfMids, sfCand, sfCount, sfSortTmp, sfFlag, sfPos, sfKp, sfKin, sfSrc,
        sfDesc, sfDW, sfAng;
    // ORB detection / description
    DevBuf orbPyr, orbTab, orbLev, orbMap, orbFlag, orbPos, orbKp, orbR, orbBlur, orbDesc, orbPat;
    std::vector<int> orbUserPattern;  // fm3d_orb_set_pattern (empty: makeRandomPattern(orbPatchSize))
    // the patch path's offset table (launch_orb_offset_table): 512 (dx, dy), the pattern, patch size and
    // keypoint angle it was built from, and its largest |offset| + 3 (0: no table; fm3d_patchdesc.cpp)
    DevBuf orbOffTab;
    std::vector<int> orbTabPattern;
    int orbTabPatchSize = 0, orbTabReach = 0;
    float orbTabAngle = 0.f;
    // SIFT detection / description
    DevBuf siftImg, siftBase, siftG, siftD, siftGL, siftDL, siftTaps, siftScan, siftFlag, siftPos, siftCand, siftAng,
        siftNpk, siftKp, siftDesc;
    // BRISK description
    DevBuf brImg, brSum, brKp, brIdx, brPat, brPairs, brDesc;
    // FREAK description (frLut: the whole default pattern, uploaded once)
    DevBuf frImg, frSum, frKp, frScale, frLut, frOp, frPairs, frAng, frDesc;
    DevBuf msImg, msWork, msHeap, msNode, msHist, msReg, msCnt, msOff, msXY, msScr, msKp, msFlag, msPos, msOut, msRank,
        msPad, msRegC;
    std::vector<int> freakUserPairs;  // fm3d_freak_set_pairs (empty: FM3D_FREAK_DEF_PAIRS)
    // STAR detection
    DevBuf starImg, starS, starT, starF, starR, starZ, starKp, starFlag, starPos, starOut, starWork;
    // NCC hypotheses over the pipeline's inliers (fm3d_pipeline_run_ncc)
    DevBuf nccS, nccN, nccB;
    int nccH = 0;
    DevBuf f32Work;           // the bf16 MFMA prefilter's scratch (rows, norms, bounds, candidates)
    int nCU = 0;
    DevBuf kp1, kp2, triPts, triMask, triMask8, pts, srcIdx;
    long lmGroups = 0;
    int wallKhz = 0;
    DevBuf lmNormals, lmStatus, lmInfo, lmNfev, lmMdat, lmQueue, lmStat, slab, slabI1;
    // the fused compactions' look-back state (fm3d_kernels.h LookBack): status words, block counter
    DevBuf lbSt, lbCtr;
    unsigned lbEpoch = 0;  // the last look-back launch's tag (fm3d_kernels.h LookBack)
    DevBuf records, recTmp, recFlag;
    DevBuf lmProj;  // camera-2 projection constants for the LM kernel (fm3d::ProjConst)
    DevBuf pcnt;    // the pipeline's device counts: [0] matches K, [1] inliers P, [2] kept
    // fm3d_pipeline_run(_dlt)_verified and the verified submits: the verification's working memory (grown
    // on demand, reused across pairs) and the compaction's output, swapped with `matches` once it holds
    // the verified ones
    DevBuf verWork, verMatches;
    // fm3d_pipeline_describe (fm3d_tail.cpp): per point the frame, R, t and descriptor row; one chunk of
    // patches (the one-shot patch descriptors borrow the last two)
    DevBuf tailFrames, tailRT, tailDesc, tailPatch;
    // the patch describer (fm3d_patchdesc.cpp): the per-patch constant tables of pdCap patches of edge
    // pdSize (centred keypoint of angle pdAngle, SiftLevel rows, level indices), the SIFT blur taps of
    // pdSigma and the oriented path's kept count
    DevBuf pdKp, pdGL, pdLvl, pdTaps, pdKept;
    int pdCap = 0, pdSize = 0, pdNTaps = 0;
    float pdAngle = 0.f, pdSigma = 0.f;
    // pinned staging: descriptors A / B (padded rows), keypoints, images, small tables, results
    HostBuf hA, hB, hK1, hK2, hImg, hTab, hProj, hSmall, hFlag;
    HostBuf hVer;  // a verified submit's fm3d::VerifySmall, stored by launch_verify_report
    hipEvent_t evStage = nullptr;  // after the last H2D copy from the staging buffers
    hipEvent_t evProj = nullptr;   // after the last H2D copy of the LM constants (hProj)
    int nccP = 0;          // points of the last successful fm3d_pipeline_run_ncc (its score rows)
    bool staged = false;
    struct Pipe {  // the staged pipeline's members (fm3d_pipeline.cpp)
        fm3d_host::PairState state = fm3d_host::PairState::Idle;
        // staged inputs
        int nA = 0, nB = 0, dim = 0, type = 0, dimPad = 0, queryOffset = 0;
        int K = 0, P = 0;      // matches and inliers of the last waited front half
        bool stageEv = true;   // the last front half recorded EV_MATCH_DONE / EV_DLT_DONE (FM3D_STAGE_EVENTS)
        fm3d_record* subOut = nullptr;   // the submitted pair's record destination (device; null: internal)
        fm3d_record* pendOut = nullptr;  // the device records of the pending / last run
        fm3d_lm_stats subLm{};           // the pending submit's LM launch data
        int nccHPending = 0;             // the pending NCC scoring's hypotheses per point
        // fm3d_pipeline_link: a member's submit queues its front half only; the leader's next submit
        // queues ONE LM launch over both pairs' points and the member's records behind it
        fm3d_ctx* linkLeader = nullptr;      // (member) the context that launches its LM
        std::vector<fm3d_ctx*> linkMembers;  // (leader) the contexts whose pairs join its launches
        hipEvent_t evFront = nullptr;        // (member) after its front half
        hipEvent_t evLm = nullptr;           // (leader) after a joint LM launch
    } pipe;
    hipEvent_t ev[fm3d_host::EV_COUNT] = {};
    std::string err;

    fm3d_ctx() = default;
    fm3d_ctx(const fm3d_ctx&) = delete;
    fm3d_ctx& operator=(const fm3d_ctx&) = delete;
    // fm3d_ctx_destroy runs this with the context's device current and its stream synchronised.  The
    // events and the owned stream are destroyed first, in this body; the buffers free themselves
    // after it, as members.  The stream is idle by then and freeing names no stream, so either
    // order would do: this one keeps the stream a plain member.
    ~fm3d_ctx() {
        for (hipEvent_t e : {evStage, evProj, pipe.evFront, pipe.evLm})
            if (e) hipEventDestroy(e);
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
        if (ownStream) hipStreamDestroy(stream);
    }
};

namespace fm3d_host {

inline int fail(fm3d_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

// an A/B switch of the environment: on unless its value starts with '0'
inline bool env_on(const char* name) {
    const char* e = getenv(name);
    return !(e && e[0] == '0');
}

// ---- fm3d_host.cpp: helpers of more than one translation unit
// the scan scratch and the count word of a compaction over n flags
int ensure_scan_tmp(fm3d_ctx* c, int n);
void install_g12(fm3d_ctx* c, const double g[16]);
bool good_max_px(double v);  // finite and > 0 (false for NaN)
// the gate's device inputs from keypoints already on the device (kp1: nA queries, kp2: nB train
// rows), queued on the context stream
int make_gate(fm3d_ctx* c, const fm3d_point2f* kp1, int nA, const fm3d_point2f* kp2, int nB, double maxPx,
              fm3d::EpiGate* g);
int ensure_offsets(fm3d_ctx* c);
int upload(fm3d_ctx* c, DevBuf& b, const void* src, size_t bytes);
int staging_wait(fm3d_ctx* c);
int upload_pinned(fm3d_ctx* c, DevBuf& dst, HostBuf& h, const void* src, size_t bytes);
// the look-back state of one fused-compaction launch of nBlocks blocks on c's stream
int make_lookback(fm3d_ctx* c, int nBlocks, fm3d::LookBack* lb);
fm3d::TriParams tri_params(fm3d_ctx* c, int K, int queryOffset);
fm3d::NccParams ncc_params(fm3d_ctx* c, int Hphi, int Htheta, double span);
int set_images_impl(fm3d_ctx* c, const uint8_t* img1, const uint8_t* img2, int width, int height, int stride,
                    bool sync = true, bool waitStaging = true);

// ---- fm3d_matching.cpp
int stage_descriptors(fm3d_ctx* c, const void* descA, int nA, const void* descB, int nB, int dim, int type,
                      int* effType, int* dimPad, bool waitStaging = true, bool speculate = false);
// run_match's options.  compactOut / compactCount (the pipeline): NNDR, the parts' merge (int keys)
// and the stable compaction of the kept matches in one launch; else the NNDR flags and candidates in
// c->flag / c->cand.  gate (fm3d_kernels.h EpiGate): every type takes its gated kernels.  crossCheck
// 1 / 2 (with compactOut only): the reverse search over the same rows (and the same
// gate, transposed), then the NNDR launch's mutual form
struct MatchOpts {
    double eps = 0.0;
    int queryOffset = 0;
    bool wantKnn = false;
    fm3d_dmatch* compactOut = nullptr;
    int* compactCount = nullptr;
    const fm3d::EpiGate* gate = nullptr;
    int crossCheck = 0;
};
int run_match(fm3d_ctx* c, int nA, int nB, int type, int dimPad, const MatchOpts& o);

// ---- fm3d_tail.cpp
int describe_chunk();  // patches per chunk: the constant, or FM3D_DESCRIBE_CHUNK clamped to 1 .. 65535

// ---- fm3d_lm.cpp
// One frame pair's points for an LM launch: its context (pyramids c->lvlDesc, pose c->R2/t2,
// outputs c->lm*, per-pair counters c->pcnt + 16 bytes) and the points (c->pts): P of them, or
// P their bound when Pdev holds the count on the device (the pipeline: no host sync)
struct LMSrc {
    fm3d_ctx* c;
    int P;
    const int* Pdev;
};
int lm_groups(fm3d_ctx* c, const void* kptr, int slots, long Ptot, long* out);
int run_lm_multi(fm3d_ctx* c, const LMSrc* src, int nProb, fm3d_lm_stats* stats, hipEvent_t e0, hipEvent_t e1);
int run_lm(fm3d_ctx* c, int P, const int* Pdev, fm3d_lm_stats* stats, hipEvent_t e0, hipEvent_t e1);
void fill_lm_cycles(const fm3d_ctx* c, const unsigned long long* cnt, fm3d_lm_stats* st);
fm3d::Camera lm_camera(const fm3d::Camera& cam);

// fm3d_pipeline_run(_dlt)_verified's middle (fm3d_verify.cpp): the verification of the K matches in
// c->matches against the staged keypoints, queued on the context stream in c->verWork; the verified
// matches, compacted, take the place of c->matches and their count that of c->pcnt[0]; with
// o->poseFromModel the pose candidates and their votes.  One host wait.  Fills rep's best, verified,
// roundsAdopted, E, votes and verify_ms; *havePose: g12 holds fm3d_pose_from_epipolar's pose (not yet
// installed).  K >= 8.
int verify_staged(fm3d_ctx* c, const fm3d_verify_opts* o, int K, fm3d_verify_report* rep, bool* havePose,
                  double g12[16]);
// The same stage for the verified submits, in filter mode (o->poseFromModel == 0), behind a queued match
// half and without a host wait: the device-count launch forms, sized by the staged nA and reading the
// match count where the match stage left it, c->pcnt[0].  The compaction puts the verified count there
// and launch_verify_report stores the match count, the verified count, best, the adopted rounds and E
// to c->hVer for the wait (verify_report).  No model: every flag is 0 and so is the verified count.
int verify_staged_queue(fm3d_ctx* c, const fm3d_verify_opts* o);
// after the stream ran verify_staged_queue: rep from c->hVer, the context's pose and the events.
// FM3D_ERR_HIP for a count outside [0, nA].
int verify_report(fm3d_ctx* c, fm3d_verify_report* rep);

}  // namespace fm3d_host

#define HIPCHK(ctx, expr)                                                                \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fm3d_host::fail((ctx), FM3D_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)
