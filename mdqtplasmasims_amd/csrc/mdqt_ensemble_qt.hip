// The batched QT kernels of an ensemble of jobs (mdqt_ensemble_substeps), in a translation unit — hence a
// code object — of their own: mdqt_qtfast.hip's, which holds the single-job kernels, stays byte for byte
// what it is without the ensemble (a larger code object cost the single-job QT launch 0.2 us of 18.5,
// measured).  The kernels wrap lane_substeps, which lives in mdqt_qtfast.hip: that file is included here
// with its own launchers compiled out and its ensemble section (the end of the file) compiled in.  Built
// with mdqt_qtfast.hip's flags (Makefile QTSCHED).
#define MDQT_ENSEMBLE_TU 1
#include "mdqt_qtfast.hip"
