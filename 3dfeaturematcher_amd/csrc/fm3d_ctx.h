// fm3d_ctx.h -- the context behind the C ABI's opaque fm3d_ctx, its self-freeing buffers and the few
// helpers that more than one translation unit of the library uses (private, like fm3d_internal.h).
#pragma once

#include <hip/hip_runtime.h>

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
        if (e == hipSuccess) bytes = alloc;
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
};
// page-locked host staging: the H2D copies of the inputs run asynchronously from it, at full PCIe
// rate, and the host may return before they execute (fm3d_pipeline_submit)
struct PinnedMem {
    static constexpr size_t kMin = 4096;
    static hipError_t alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
};
using DevBuf = Buf<DeviceMem>;
using HostBuf = Buf<PinnedMem>;

constexpr size_t kGuard(int w) { return (size_t)4 * w + 64; }

// the pipeline's small device -> host results of one frame pair (one D2H, pinned)
struct PipeSmall {
    int32_t cnt[4];                 // matches K, inliers P, kept, pad (c->pcnt bytes 0..15)
    unsigned long long prob[2];     // this pair's residual / pixel evaluations (c->pcnt bytes 16..31)
    unsigned long long lm[26];      // the LM launch's counters (fm3d_lm2.hip statPass layout)
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
    int pyrGuardW = -1, pyrGuardH = -1, pyrGuardLevels = -1;  // the geometry whose guards are zero
    DevBuf lvlDesc;
    // circle offsets of pixelsRay
    DevBuf offsets;
    int nOff = 0, nOffPad = 0;
    // work buffers
    DevBuf A, B, cqA, ctB, idx, key, fkey, knnOut, cand, flag, matches, count, scanTmp;
    DevBuf partIdx, partKey;  // per-part top-2 lists of the split matchers
    DevBuf A8, B8;            // binary rows unpacked to int8 for the MFMA matcher; u8 rows packed from floats
    DevBuf u8Flag;            // launch_f32_pack_u8's "not integer-valued" flag
    // the guided matchers' gate (fm3d_kernels.h EpiGate): query lines (float4) and train (u, v)
    DevBuf gLines, gUV;
    bool gateStaged = false;  // they belong to the staged pair's keypoints under the current g12
    // the cross-check's reverse search (KnnSide): allocated only when it runs
    DevBuf rCq, rCt, rA8, rB8, rPartIdx, rPartKey, rPairs, rIdx, rKey, rFkey;
    bool specU8 = false;      // the staged float rows went to the u8 matcher before their flag was read
    // SURF detection / description
    DevBuf sfImg, sfSum, sfDet, sfTr, sfLayers, sfMids, sfCand, sfCount, sfSortTmp, sfFlag, sfPos, sfKp, sfKin, sfSrc,
        sfDesc, sfDW, sfAng;
    // ORB detection / description
    DevBuf orbPyr, orbTab, orbLev, orbMap, orbFlag, orbPos, orbKp, orbR, orbBlur, orbDesc, orbPat;
    std::vector<int> orbUserPattern;  // fm3d_orb_set_pattern (empty: makeRandomPattern(orbPatchSize))
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
    DevBuf bPairs;            // the f32 train rows in interleaved pairs
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
    // fm3d_pipeline_run(_dlt)_verified: the verification's working memory (grown on demand, reused across
    // pairs) and the compaction's output, swapped with `matches` once it holds the verified ones
    DevBuf verWork, verMatches;
    // pinned staging: descriptors A / B (padded rows), keypoints, images, small tables, results
    HostBuf hA, hB, hK1, hK2, hImg, hTab, hProj, hSmall, hFlag;
    hipEvent_t evStage = nullptr;  // after the last H2D copy from the staging buffers
    hipEvent_t evProj = nullptr;   // after the last H2D copy of the LM constants (hProj)
    bool pending = false;          // a fm3d_pipeline_submit awaiting fm3d_pipeline_wait
    // fm3d_pipeline_link: a member's submit queues its front half only; the leader's next submit
    // queues ONE LM launch over both pairs' points and the member's records behind it
    fm3d_ctx* linkLeader = nullptr;        // (member) the context that launches its LM
    std::vector<fm3d_ctx*> linkMembers;    // (leader) the contexts whose pairs join its launches
    bool frontOnly = false;          // (member) submitted, its LM not queued yet
    fm3d_record* subOut = nullptr;   // the submitted pair's record destination (device; null: internal)
    hipEvent_t evFront = nullptr;    // (member) after its front half
    hipEvent_t evLm = nullptr;       // (leader) after a joint LM launch
    fm3d_lm_stats subLm{};         // the pending submit's LM launch data
    bool pendingDlt = false;       // the pending submit is fm3d_pipeline_submit_dlt's front half
    bool pendingNcc = false;       // the pending submit is fm3d_pipeline_submit_ncc's front half + NCC
    int nccHPending = 0;           // its hypotheses per point
    fm3d_record* pendOut = nullptr;  // the device records of the pending / last run
    // staged pipeline inputs
    int stNA = 0, stNB = 0, stDim = 0, stType = 0, stDimPad = 0, stQueryOffset = 0;
    int stK = 0, stP = 0;  // matches and inliers of the last fm3d_pipeline_run_dlt
    bool stageEv = true;   // the last pipeline_front recorded ev[3] / ev[5] (FM3D_STAGE_EVENTS)
    int* frontHostCnt = nullptr;  // pipeline_front: the DLT kernel also stores (K, P) here (device pointer)
    int nccP = 0;          // points of the last successful fm3d_pipeline_run_ncc (its score rows)
    bool staged = false;
    // [0..1] standalone LM, [2..7] pipeline stages ([4] and [9]: around the verification of
    // fm3d_pipeline_run_verified), [8] submit start, [1] end
    hipEvent_t ev[10] = {};
    std::string err;

    fm3d_ctx() = default;
    fm3d_ctx(const fm3d_ctx&) = delete;
    fm3d_ctx& operator=(const fm3d_ctx&) = delete;
    // fm3d_ctx_destroy runs this with the context's device current and its stream synchronised.  The
    // events and the owned stream are destroyed first, in this body; the buffers free themselves
    // after it, as members.  The stream is idle by then and freeing names no stream, so either
    // order would do: this one keeps the stream a plain member.
    ~fm3d_ctx() {
        for (hipEvent_t e : {evStage, evProj, evFront, evLm})
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

// the scan scratch and the count word of a compaction over n flags (fm3d_host.cpp)
int ensure_scan_tmp(fm3d_ctx* c, int n);

// fm3d_pipeline_run(_dlt)_verified's middle (fm3d_verify.cpp): the verification of the K matches in
// c->matches against the staged keypoints, queued on the context stream in c->verWork; the verified
// matches, compacted, take the place of c->matches and their count that of c->pcnt[0]; with
// o->poseFromModel the pose candidates and their votes.  One host wait.  Fills rep's best, verified,
// roundsAdopted, E, votes and verify_ms; *havePose: g12 holds fm3d_pose_from_epipolar's pose (not yet
// installed).  K >= 8.
int verify_staged(fm3d_ctx* c, const fm3d_verify_opts* o, int K, fm3d_verify_report* rep, bool* havePose,
                  double g12[16]);

}  // namespace fm3d_host

#define HIPCHK(ctx, expr)                                                                \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fm3d_host::fail((ctx), FM3D_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)
