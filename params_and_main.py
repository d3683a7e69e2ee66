"""Configuration + driver of the tile workflow (reference ``params_and_main.py:21-180``) on the MI355X hot path.

Edit the globals, then run ``python params_and_main.py``.  ``Create_tiles`` is CPU preprocessing (``create_tiles_unet.py``, numpy + unet_amd.tiffio instead of GDAL/rasterio);
``Train`` and ``Predict`` run on the GPU.
"""
from __future__ import annotations

import time

from unet_amd import xresnet18, xresnet34, xresnet34_deep, xresnet50, xresnet101  # noqa: F401

# ----------------------------------------------------------------------------------- switches (params_and_main.py:22-24)
Create_tiles = True
Train = False
Predict = False

# ----------------------------------------------------------------------------------- tiles (params_and_main.py:31-38)
image_path = "PATH"
mask_path = "PATH"             # None when cutting prediction tiles without a mask
base_dir = "PATH"
patch_size = 400
patch_overlap = 0              # 0.2 with split = [1] to cut prediction tiles of a full image
split = [0.8, 0.2]

# ----------------------------------------------------------------------------------- training (params_and_main.py:45-63)
data_path = base_dir
model_path = "PATH"
description = "Beschirmung_geo_Aug_data"
info = "RGB images"
existing_model = None          # or the path of an exported model: transfer learning
BATCH_SIZE = 4                 # the reference's value for a 16 GB P100; 16 fits an MI355X many times over
EPOCHS = 15
LEARNING_RATE = 0.0001
enable_regression = False
visualize_data_example = True  # plots are out of scope on this path (ignored)
export_model_summary = True
CODES = ["NO_Data", "Background", "Beschirmung"]
CLASS_WEIGHTS = "even"         # list, "even" or "weighted"

# ----------------------------------------------------------------------------------- prediction (params_and_main.py:68-76)
predict_path = "PATH"
predict_model = "PATH"         # model_path/description/description.pkl
AOI = "str"
year = "str"
merge = False
regression = False
validation_vision = True       # confusion-matrix figures: out of scope on this path (ignored)

# ----------------------------------------------------------------------------------- extra parameters (params_and_main.py:84-118)
enable_extra_parameters = True
self_attention = True
ENCODER_FACTOR = 10
LR_FINDER = None               # None, "minimum", "steep", "valley", "slide"
VALID_SCENES = ["vali"]
loss_func = None               # None = CrossEntropyLossFlat(axis=1) (the reference's default object) | FocalLossFlat(gamma=2, axis=1) | DiceLoss(axis=1) | CombinedLoss(axis=1) (from unet_amd.learner);
                               # regression: MSELossFlat(axis=1), L1LossFlat
                               # BorderWeightedCrossEntropy(axis=1, w0=10, sigma=5, exclude=None): the U-Net paper's cross-entropy with a per-pixel
                               # weight that is large near class borders (thin gaps between crowns, roofs, parcels); exclude=0 with class_zero
                               # LOSS_FUNCTION (loss_func here) = BorderWeightedCrossEntropy(objects=True): the paper's own (d1 + d2) form -- the weight is large only
                               # on background pixels between two different objects (background=0, radius=None = ceil(6 sigma) px)
monitor = "valid_loss"         # 'dice_multi', 'r2_score', 'train_loss', 'valid_loss'
all_classes = False
specific_class = None
large_file = False
max_empty = 0.2
class_zero = False
ARCHITECTURE = xresnet34
transforms = True
split_idx = 0
n_transform_imgs = 1
# None = the reference's default pipeline HorizontalFlip(p=0.5) + VerticalFlip(p=0.5); or, with `from unet_amd import augment as A`:
# A.Compose([A.HorizontalFlip(p=0.5), A.VerticalFlip(p=0.5),
#            A.RandomBrightnessContrast(brightness_limit=(-0.1, 0.1), contrast_limit=(-0.1, 0.1), p=0.5), A.CoarseDropout(p=0.5)])
# Geometric: A.RandomRotate90(p=0.5), A.Transpose(p=0.5), A.Rotate(limit=90, p=0.5), A.ShiftScaleRotate(p=0.5) (square tiles for the first two)
aug_pipe = None
# test-time augmentation of Predict: None | "flips" (4 passes, any tile shape) | "d4" (8 passes, square tiles) | a tuple of D4 codes
# (unet_amd/tta.py); every tile's probabilities become the mean over the flipped / rotated passes, mapped back
TTA = None
# how the windows of a merged prediction (merge = True) combine: "mean" (the reference's unweighted mean) | "gaussian" (each window
# weighted with a centre-peaked Gaussian importance map, sigma = tile size / 8: the seams where windows end fade; not with large_file)
BLEND = "mean"
# clean-up of the merged class mask on the GPU before it is written (merge = True, class output): None | a dict of
# unet_amd.postprocess.PostProcess arguments, e.g. {"majority": 5, "sieve": 64} = a 5 x 5 majority filter, then a sieve that merges
# regions under 64 px into their largest neighbour ("connectivity": 4 | 8; with class_zero set "frozen_class": 0 to keep NO_Data as it is)
POSTPROCESS = None
# compression of the prediction outputs: None (uncompressed, one strip) | "lzw" (LZW strips; the merged raster is encoded on the GPU and
# only the compressed bytes reach the host) | ("lzw", 2) to add horizontal differencing (Predictor 2, class / integer outputs only)
COMPRESS = None
# layout of the merged prediction raster (needs COMPRESS): TILE None (strips) | a multiple of 16 in 16..1024, 256 being the usual choice
# (square LZW tiles); OVERVIEWS None | "auto" | "mode" | "average" | "nearest" (needs TILE): the overview pyramid behind the full-resolution
# image, i.e. a cloud-optimised GeoTIFF -- "auto" takes "mode" for class masks and "average" for everything else
TILE = None
OVERVIEWS = None
# polygons of the merged class mask (merge = True, class output), traced on the GPU and written as <merged raster stem>.geojson: VECTOR
# False | True; VECTOR_EXCLUDE None | a class id | a list of class ids that get no polygon (with class_zero, NO_Data never gets one)
VECTOR = False
VECTOR_EXCLUDE = None
# VECTOR_SIMPLIFY None | a tolerance in pixels (0..4096): the rings are simplified on the GPU (Douglas-Peucker per shared border, so that
# neighbouring polygons keep one common border) before they are written
VECTOR_SIMPLIFY = None
# touching objects of a class split into instances on the GPU (merge = True, class output; needs VECTOR, INSTANCES_RASTER or both): INSTANCES
# None | a dict of unet_amd.instances.Instances arguments, e.g. {"classes": [2], "radius": 64, "min_depth": 2.0} = split class 2 along the
# ridges of its distance transform (capped at 64 px) and merge basins shallower than 2 px back; the GeoJSON then has one feature per
# instance.  INSTANCES_RASTER False | True: <merged raster stem>_instances.tif, a uint32 raster of the instance ids (0 off the split classes)
INSTANCES = None
INSTANCES_RASTER = False
# zonal statistics of the merged class mask (merge = True, class output), counted on the GPU (unet_amd/zonal.py): ZONES None | the path of a
# GeoJSON file of Polygon / MultiPolygon zones (parcels, districts, stands) in the raster's coordinates; the pixels and the share of every
# class per zone are written as <merged raster stem>_zonal.geojson with the zones' own properties.  ZONAL_OBJECTS False | True: also the
# number of objects (components, or the instances of INSTANCES) per zone and class; an object counts in the zone of its first pixel
ZONES = None
ZONAL_OBJECTS = False
# ZONAL_VALUES False | True (needs ZONES, merge = True and a float output: regression or specific_class): the table holds pixels, area, valid,
# mean, std, min, max and sum of the predicted float plane per zone -- mean predicted cover per parcel -- instead of the class counts
ZONAL_VALUES = False
# attributes of every object of the merged class mask (merge = True, class output), measured on the GPU (unet_amd/objects.py): OBJECTS False |
# True writes <merged raster stem>_objects.geojson, one point per object (component, or instance of INSTANCES) inside it, with pixels, area,
# perimeter, centroid, bbox, diameter, compactness and on_edge -- a tree list with crown diameters; with VECTOR the polygons carry the same
# attributes.  OBJECTS_EXCLUDE None | class id | list of class ids whose objects are not measured
OBJECTS = False
OBJECTS_EXCLUDE = None
# a value per object (needs OBJECTS): OBJECTS_VALUES None | the path of a one-band GeoTIFF on the merged raster's grid (a canopy height model,
# an NDVI): every object gains <OBJECTS_VALUES_NAME>_valid, _mean, _std, _sum, _min, _max and _peak_x, _peak_y, the place where the value peaks
# (tree height and treetop).  OBJECTS_CONFIDENCE False | True: the same of the merged probability of the predicted class, as confidence_*
OBJECTS_VALUES = None
OBJECTS_VALUES_NAME = "value"
OBJECTS_CONFIDENCE = False
# a mask_path that ends in .geojson / .json holds polygons instead of a raster: Create_tiles burns them on the GPU onto the image's grid
# (unet_amd/rasterize.py) with this integer property as the class id
MASK_ATTRIBUTE = "class"


def main():
    global large_file, specific_class, all_classes, transforms, VALID_SCENES, self_attention, monitor, loss_func, LR_FINDER
    global ENCODER_FACTOR, ARCHITECTURE, enable_regression, max_empty, TTA, BLEND, POSTPROCESS, COMPRESS, TILE, OVERVIEWS
    global VECTOR, VECTOR_EXCLUDE, VECTOR_SIMPLIFY, INSTANCES, INSTANCES_RASTER, ZONES, ZONAL_OBJECTS, OBJECTS, OBJECTS_EXCLUDE
    global ZONAL_VALUES, OBJECTS_VALUES, OBJECTS_VALUES_NAME, OBJECTS_CONFIDENCE
    t0 = time.time()
    if enable_extra_parameters:          # params_and_main.py:129-145
        import warnings
        warnings.warn("Extra parameters are enabled. Code may behave in unexpected ways. "
                      "Please disable unless experienced with the code.")
    else:
        ENCODER_FACTOR, LR_FINDER, VALID_SCENES, loss_func, monitor = 10, None, ["vali"], None, None
        all_classes, specific_class, enable_regression, large_file, max_empty = False, None, False, False, 0.9
        ARCHITECTURE, self_attention = xresnet34, False
        TTA, BLEND, POSTPROCESS, COMPRESS, TILE, OVERVIEWS = None, "mean", None, None, None, None
        VECTOR, VECTOR_EXCLUDE, VECTOR_SIMPLIFY = False, None, None
        INSTANCES, INSTANCES_RASTER = None, False
        ZONES, ZONAL_OBJECTS, ZONAL_VALUES = None, False, False
        OBJECTS, OBJECTS_EXCLUDE = False, None
        OBJECTS_VALUES, OBJECTS_VALUES_NAME, OBJECTS_CONFIDENCE = None, "value", False
    if Create_tiles:
        from create_tiles_unet import split_raster
        split_raster(path_to_raster=image_path, path_to_mask=mask_path, base_dir=base_dir, patch_size=patch_size,
                     patch_overlap=patch_overlap, split=split, max_empty=max_empty, class_zero=class_zero, mask_attribute=MASK_ATTRIBUTE)
    if Train:
        from train import train_func
        train_func(data_path, existing_model, model_path, description, BATCH_SIZE, visualize_data_example, enable_regression,
                   CLASS_WEIGHTS, ARCHITECTURE, EPOCHS, LEARNING_RATE, ENCODER_FACTOR, LR_FINDER, loss_func, monitor, self_attention,
                   VALID_SCENES, CODES, transforms, split_idx, export_model_summary, aug_pipe, n_transform_imgs, info, class_zero)
    if Predict:
        from predict import save_predictions
        extra = {} if BLEND == "mean" else {"blend": BLEND}
        if POSTPROCESS is not None:
            extra["postprocess"] = POSTPROCESS
        if COMPRESS is not None:
            extra["compress"], extra["predictor"] = COMPRESS if isinstance(COMPRESS, tuple) else (COMPRESS, 1)
        if TILE is not None:
            extra["tile"] = TILE
        if OVERVIEWS is not None:
            extra["overviews"] = OVERVIEWS
        if VECTOR:
            extra["vector"], extra["vector_exclude"] = True, VECTOR_EXCLUDE
            if VECTOR_SIMPLIFY is not None:
                extra["vector_simplify"] = VECTOR_SIMPLIFY
        if INSTANCES is not None:
            extra["instances"], extra["instances_raster"] = INSTANCES, INSTANCES_RASTER
        if ZONES is not None:
            extra["zones"], extra["zonal_objects"] = ZONES, ZONAL_OBJECTS
        if ZONAL_VALUES:
            extra["zonal_values"] = True
        if OBJECTS:
            extra["objects"], extra["objects_exclude"] = True, OBJECTS_EXCLUDE
        if OBJECTS_VALUES is not None:
            extra["objects_values"], extra["objects_values_name"] = OBJECTS_VALUES, OBJECTS_VALUES_NAME
        if OBJECTS_CONFIDENCE:
            extra["objects_confidence"] = True
        save_predictions(predict_model, predict_path, regression, merge, all_classes, specific_class, large_file, AOI, year,
                         validation_vision, class_zero, tta=TTA, **extra)
    print(f"Operation completed in {(time.time() - t0) / 60:.2f} minutes.")


if __name__ == "__main__":
    main()
