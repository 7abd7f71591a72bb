// What the wrappers of the ptgpp-compiled solver taskpools (*_jdf.cpp) share:
// the info words, the arena of the diagonal-block inverses, the start-empty
// gate, composition that owns its parts, and the argument checks.
#pragma once
#include <initializer_list>

#include "../data/collections.hpp"
#include "../ptg/ptg.hpp"

namespace parsec {
namespace algos {

// The info words of one generated taskpool: `dev` is a pooled device status word
// (no hipMalloc / hipMemset / hipFree per taskpool; null without a GPU), `cpu` the
// word of the CPU bodies. Both receive the 1-based global index k * nb + i of a
// failing diagonal entry.
struct InfoWords {
  int gpu;
  int* dev;
  int* cpu;
  int* hip() const { return dev ? dev : cpu; }  // what the JDF's INFO global takes
};
// The generated _new functions take the two words as arguments: acquire them
// before the call, attach them to the taskpool it returned.
InfoWords info_acquire();
// On completion *info_host (optional) receives the smaller non-zero of the two
// words and the device word goes back to the pool; the taskpool's destructor
// frees the host word (and the device word of a taskpool that never ran).
void info_attach(ptg::PtgTaskpool* tp, InfoWords w, int* info_host);

// The arena of the inverses of the 64 x 64 diagonal blocks of one nb x nb tile.
void inv_arena(ArenaDatatype& adt, int64_t nb);

// Start-empty gate: *gate is read when tp is enqueued, and non-zero sets *extent
// (the hidden global that bounds every task range of the JDF, _g_MT or _g_NT) to
// 0, so the taskpool starts with no task at all. A null gate installs nothing.
void gate_on(Taskpool* tp, const int* gate, int* extent);

// The parts run one after the other as one taskpool of that name; freeing it
// (taskpool_free) frees the parts.
Taskpool* compose_owned(const char* name, std::initializer_list<Taskpool*> parts);

// Argument checks: the reason a request is refused, or nullptr.
// A is a square double matrix with square tiles (the factor of DPOTRF / DGETRF_NOPIV)
const char* factor_problem(const TiledMatrix* A);
// ... and B a right-hand side for it: as many rows as A, B->mb == A->nb
const char* solve_problem(const TiledMatrix* A, const TiledMatrix* B);
// A and its companion L for the tile LU with incremental pivoting: A as for
// factor_problem with a tile of at most 1024, L of the same type, tile size
// (nb x nb), tile grid and distribution
const char* incpiv_problem(const TiledMatrix* A, const TiledMatrix* L);
// A (M x N, square tiles) and T hold a tile QR factor, B has M rows and B->mb == A->mb
const char* qr_solve_problem(const TiledMatrix* A, const TiledMatrix* T, const TiledMatrix* B);

}  // namespace algos
}  // namespace parsec
