// Reference: src/postprocess.cpp:47 (header-less there; textually included at src/process.cpp:9).
#pragma once
#include "../mi_unet.h"
#include "image.h"

// hole fill (components of mask != 2 that touch no image edge and are smaller than 6 % of the image) -> 3x3 open of
// (mask == 2) -> keep 8-connected components of at least 6 % of the image -> output in {0, 2}.
medseg::Image8 postprocess_mask(const medseg::Image8 &src);

// The same chain for any class and area rule (a target of include/mi_unet.h): `== cls` in place of `== 2`, min_area =
// mi_unet_target_min_area(rows, cols, min_area_frac) in place of 6 %; output in {0, cls}.  postprocess_mask(src) is
// postprocess_mask(src, 2, 0.06f).
medseg::Image8 postprocess_mask(const medseg::Image8 &src, int cls, float min_area_frac);

// ... and for any morphology (mi_unet_morph in include/mi_unet.h): hole fill -> close by the element of radius close_r
// -> open by the element of radius open_r -> area filter, the element a box or a Euclidean disc, the border neither constraining an
// erosion nor seeding a dilation.  The two overloads above are this one at { MI_UNET_MORPH_RECT, 1, 0 }.  Throws for an unknown shape or
// a radius outside 0 .. MI_UNET_MORPH_MAX_R.
medseg::Image8 postprocess_mask(const medseg::Image8 &src, int cls, float min_area_frac, const mi_unet_morph &morph);
