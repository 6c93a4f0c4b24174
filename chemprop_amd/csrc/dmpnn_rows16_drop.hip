// The per-step split-MFMA contraction (dmpnn_rows16_impl.hpp) with the dropout mask in its epilogue: block dropout of the per-step
// general route on the f16 pipe (dmpnn_fwd_args.dropout_p) and dmpnn_linear16_dropout_fwd.  The builds live in a translation unit
// of their own so that they compile beside the plain ones (dmpnn_rows16.hip), which launches them.
#include "dmpnn_rows16_impl.hpp"

namespace dmpnn {
namespace rows16 {
DMPNN_DEFINE_ROWS16_DROP(1, 4)
DMPNN_DEFINE_ROWS16_DROP(2, 4)
DMPNN_DEFINE_ROWS16_DROP(3, 4)
DMPNN_DEFINE_ROWS16_DROP(4, 4)
DMPNN_DEFINE_ROWS16_DROP(5, 4)
DMPNN_DEFINE_ROWS16_DROP(1, 12)
DMPNN_DEFINE_ROWS16_DROP(2, 12)
DMPNN_DEFINE_ROWS16_DROP(3, 12)
DMPNN_DEFINE_ROWS16_DROP(4, 12)
DMPNN_DEFINE_ROWS16_DROP(5, 12)
}  // namespace rows16
}  // namespace dmpnn
