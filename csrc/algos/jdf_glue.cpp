#include "jdf_glue.hpp"

#include <memory>
#include <vector>

#include "../device/device.hpp"
#include "../kernels/kernels.hpp"

namespace parsec {
namespace algos {

InfoWords info_acquire() {
  const int gpu = first_gpu_device_index();
  return {gpu, gpu >= 0 ? device_status_acquire(gpu) : nullptr, new int(0)};
}

void info_attach(ptg::PtgTaskpool* tp, InfoWords w, int* info_host) {
  auto released = std::make_shared<bool>(false);
  tp->complete_hook = [=] {
    int v = __atomic_load_n(w.cpu, __ATOMIC_ACQUIRE);
    if (w.dev && !*released) {
      const int dv = device_status_release(w.gpu, w.dev);  // every kernel of the taskpool has completed
      *released = true;
      if (dv && (!v || dv < v)) v = dv;
    }
    if (info_host) *info_host = v;
  };
  auto prev = tp->destructor_hook;
  tp->destructor_hook = [=] {
    if (w.dev && !*released) device_status_release(w.gpu, w.dev);
    delete w.cpu;
    if (prev) prev();
  };
}

void inv_arena(ArenaDatatype& adt, int64_t nb) { add2arena_rect(adt, sizeof(double), 4096, (nb + 63) / 64, 4096); }

void gate_on(Taskpool* tp, const int* gate, int* extent) {
  if (!gate) return;
  tp->on_enqueue = [gate, extent](Taskpool*) {
    if (__atomic_load_n(gate, __ATOMIC_ACQUIRE) != 0) *extent = 0;
    return 0;
  };
}

Taskpool* compose_owned(const char* name, std::initializer_list<Taskpool*> parts) {
  Taskpool* c = nullptr;
  for (Taskpool* p : parts) c = c ? compose(c, p) : p;
  c->taskpool_name = name;
  c->destructor_hook = [owned = std::vector<Taskpool*>(parts)] {
    for (Taskpool* p : owned) taskpool_free(p);
  };
  return c;
}

const char* factor_problem(const TiledMatrix* A) {
  if (!A) return "null matrix";
  if (A->mtype != MATRIX_DOUBLE) return "double precision matrices only";
  if (A->mb != A->nb) return "A needs square tiles";
  if (A->m != A->n) return "A must be square";
  return nullptr;
}

const char* solve_problem(const TiledMatrix* A, const TiledMatrix* B) {
  if (const char* why = factor_problem(A)) return why;
  if (!B) return "null matrix";
  if (B->mtype != MATRIX_DOUBLE) return "double precision matrices only";
  if (B->m != A->n) return "B must have as many rows as A";
  if (B->mb != A->nb) return "B's tile rows (mb) must equal A's tile size (nb)";
  return nullptr;
}

const char* incpiv_problem(const TiledMatrix* A, const TiledMatrix* L) {
  if (const char* why = factor_problem(A)) return why;
  if (A->nb > kern::kLuMaxTile) return "the tile size exceeds 1024 (the pivoted tile kernels hold a strip's rows in registers)";
  if (!L) return "null matrix";
  if (L->mtype != MATRIX_DOUBLE) return "double precision matrices only";
  if (L->mb != A->nb || L->nb != A->nb || L->mt != A->mt || L->nt != A->nt) return "L must be tiled like A (nb x nb tiles, one per tile of A)";
  if (L->nodes != A->nodes) return "L must be distributed like A";
  for (int64_t m = 0; m < A->mt; ++m)
    for (int64_t n = 0; n <= m && n < A->nt; ++n) {
      const int64_t idx[2] = {m, n};
      if (L->rank_of(idx, 2) != A->rank_of(idx, 2)) return "L must be distributed like A";
    }
  return nullptr;
}

const char* qr_solve_problem(const TiledMatrix* A, const TiledMatrix* T, const TiledMatrix* B) {
  if (!A || !T || !B) return "null matrix";
  if (A->mtype != MATRIX_DOUBLE || T->mtype != MATRIX_DOUBLE || B->mtype != MATRIX_DOUBLE) return "double precision matrices only";
  if (A->mb != A->nb) return "A needs square tiles";
  if (T->mb != A->nb || T->nb != A->nb || T->mt != A->mt || T->nt != A->nt) return "T must be tiled like A (nb x nb tiles, one per tile of A)";
  if (B->m != A->m) return "B must have as many rows as A";
  if (B->mb != A->mb) return "B's tile rows (mb) must equal A's tile size";
  return nullptr;
}

}  // namespace algos
}  // namespace parsec
