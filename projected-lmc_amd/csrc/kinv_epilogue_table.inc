// kinv_epilogue_table.inc -- the gradient epilogue of a table family F (CovFamily) with dimension capacity DC: textually included by
// k_kinv_grad_add (256 threads) and by kinv_tile_epilogue_add (the halves of k_kinv_grad_add_bf3), which name what the bodies use.
  if constexpr (F == COV_PER) {
#include "kinv_epilogue_per.inc"
  } else if constexpr (F == COV_LPER) {
#include "kinv_epilogue_lper.inc"
  } else if constexpr (F == COV_SUM) {
#include "kinv_epilogue_sum.inc"
  } else if constexpr (F == COV_RQ) {
#include "kinv_epilogue_rq.inc"
  } else if constexpr (F == COV_DOT) {
#include "kinv_epilogue_dot.inc"
  } else if constexpr (F == COV_SM) {
#include "kinv_epilogue_sm.inc"
  } else {
#include "kinv_epilogue_add.inc"
  }
