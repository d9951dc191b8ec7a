// fm3d_features.h -- what the feature translation units (fm3d_features.cpp, fm3d_feat_*.cpp, fm3d_patchdesc.cpp)
// and fm3d_pipeline_describe (fm3d_tail.cpp) call in each other (private, like fm3d_ctx.h).
#pragma once

#include <algorithm>  // the standard headers every feature file uses
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "fm3d_ctx.h"

namespace fm3d_host {

// ---- fm3d_feat_surf.cpp
const fm3d::SurfOri& surf_ori();  // SURFInvoker's orientation disc
int ensure_surf_dw(fm3d_ctx* c);  // c->sfDW: surf_dw(), uploaded once (the first use waits)

// ---- fm3d_feat_orb.cpp
int orb_retain_best(fm3d_keypoint* k, int n, int npts);  // KeyPointsFilter::retainBest
std::vector<int> orb_pattern(const fm3d_ctx* c, int patchSize);
fm3d::OrbBlurK orb_blur_kernel();
int orb_check_settings(fm3d_ctx* c);
int fast_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, int thr, bool nonmax, std::vector<fm3d_keypoint>& k);

// ---- fm3d_feat_sift.cpp
// getGaussianKernel(cvRound(sigma*8+1)|1, sigma, CV_32F), or the refusal of more taps than the blur tile holds
int sift_blur_taps(fm3d_ctx* c, double sigma, std::vector<float>& taps);
int sift_check_settings(fm3d_ctx* c);

// ---- fm3d_feat_binary.cpp
// the border BRISK's and FREAK's compute demand around a keypoint of this size: brisk::size_of of its
// scale, freak::pattern().sizes of its scale
int brisk_border(float kpSize);
int freak_border(float kpSize);

// ---- fm3d_feat_regions.cpp
int star_detect(fm3d_ctx* c, const uint8_t* img, int w, int h, int maxSize, int respThr, int lineProj, int lineBin,
                int supp, std::vector<fm3d_keypoint>& k);
fm3d::MserParams mser_params(int delta, int minArea, int maxArea, double maxVariation, double minDiversity);
int mser_detect(fm3d_ctx* c, const uint8_t* img, int count, int w, int h, const fm3d::MserParams& P,
                std::vector<fm3d_keypoint>& k, std::vector<int>& per);

// ---- fm3d_patchdesc.cpp: m equal-sized patches on the device -> m descriptor rows on the device
struct PatchDesc {  // settled once per call, before any launch
    // Binary: BRISK and FREAK, which have no batched form (patch_desc_prepare refuses an edge at which
    // they keep the centred keypoint; below it the caller's rows stay zero and nothing is queued)
    enum Kind { SurfUpright, SurfOriented, Sift, Orb, Binary } kind;
    int size, cols, type;  // patch edge (patch_desc_prepare); fm3d_descriptor_info
    size_t rowBytes;
};
// the centred keypoint of a patch, descriptorsmatcher.cpp:146-158: (center, center), center =
// (int)floor(size / 2), size = the patch edge, response 1, octave 0, class_id 0; the reference's angle is -1
fm3d_keypoint patch_keypoint(int size, float angle);
// the settings' extractor as a kind with its row format, or the refusal of the entry point (`any`
// admits the binary extractors); touches no device
int patch_desc_kind(fm3d_ctx* c, bool any, PatchDesc* d);
// Every other host-side check and refusal, the first-use tables (centred keypoints, SiftLevel rows,
// level indices, SIFT taps, sfDW, ORB's offset table and border guard) and the scratch for `cap`
// patches of edge `size`.  May wait for an upload; queues nothing that depends on the patches.
int patch_desc_prepare(fm3d_ctx* c, int size, int cap, PatchDesc* d);
// Launches only, on c->stream, no wait: patches p0 .. p0 + m of the call (m <= cap, chunks in order from
// p0 = 0) to their rows of rowsDev.  SurfOriented sums its kept counts in c->pdKept, zeroed at p0 = 0:
// the caller reads it behind its last chunk and refuses if != its total.
int patch_desc_queue(fm3d_ctx* c, const PatchDesc& d, const uint8_t* patchesDev, int p0, int m, void* rowsDev);

}  // namespace fm3d_host
