// The projection-matrix pooling (geom_pool_features_proj_* / geom_pool_features_ragged_proj_*) as a
// translation unit of its own: pooling.hip's bodies, stated there once, instantiated for MX = true, and the four matrix entry
// points at that file's end.  Why a second unit and not four more instantiations inside pooling.hip is said at its entry points.
#define GEOM_POOL_MATRIX_UNIT 1
#include "pooling.hip"
