// The explanation kernels of an oblivious handle with category sets (tahoe_oblivious_forest_create_cat): the CAT == true
// instantiations of oblivious_shap.hip's kernels and their launches, a translation unit of its own so that the two halves compile
// side by side.  With the macro defined that file gives its device code and nothing of its host code.
#define TAHOE_OBLIVIOUS_SHAP_CAT_UNIT 1
#include "oblivious_shap.hip"
