// Read-only view of an extractor handle's pyramid of the LAST call, for units outside extractor.hip that read
// mvImagePyramid (Frame::ComputeStereoMatches, stereo.hip).  Filled by extractor_pyramid_view (extractor.hip) without
// touching the device: in direct mode level 0 is NOT materialised, the view points at the last call's own image.
// What the view guarantees of a padded plane is its w x h interior and 3 px of REFLECT_101 border around it: the resize
// chain writes no more (the rest of the 19-px border exists only after a getter of mvImagePyramid asked for it).  Readers
// stay inside the image (stereo.hip checks every window against w and h before it reads).
#pragma once

#include "common.h"

namespace orbgpu {

struct PyramidView {
    int device_id;
    int nlevels;
    float scale_factor;
    int last_batch;  // frames of the last call (0: no last call)
    int w[ORBGPU_MAX_LEVELS], h[ORBGPU_MAX_LEVELS], pitch[ORBGPU_MAX_LEVELS];
    int plane_off[ORBGPU_MAX_LEVELS];  // byte offset of the padded plane inside one frame's block
    float scale[ORBGPU_MAX_LEVELS], inv_scale[ORBGPU_MAX_LEVELS];  // mvScaleFactors / mvInvScaleFactors
    const uint8_t *pyr;  // padded planes: pixel (x, y) of level l, frame f at pyr + f * frame_pyr + plane_off[l] +
    size_t frame_pyr;    //   (y + border) * pitch[l] + x + border
    int border;
    // level 0 of the last call when it ran in direct mode (direct != 0): pixel (x, y) of frame f at
    // l0 + f * l0_frame_stride + y * l0_pitch + x; otherwise level 0 is the padded plane like every other level
    const uint8_t *l0;
    size_t l0_frame_stride;
    size_t l0_pitch;
    int direct;
    DevBuf *scratch;  // device scratch owned by the handle for readers of the view (grow-only, freed with the handle)
};

int extractor_pyramid_view(const orbgpu_extractor *e, PyramidView *v);

} // namespace orbgpu
