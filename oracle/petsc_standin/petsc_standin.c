/*
 * petsc_standin.c -- a serial, one-rank stand-in for the PETSc / MPI entry
 * points that the reference's hot-path sources call (pic1dp_global, wtimer,
 * pic1dp_field, pic1dp_particle, pic1dp_interaction), and nothing more.
 *
 * TEST INFRASTRUCTURE ONLY: it lets those sources compile and run where they
 * lie (oracle/Makefile, target ref), so that the arithmetic the oracle is
 * compared with is the reference's own statements.
 *
 * Fortran calling convention: lower-case name with a trailing underscore,
 * every argument by reference, a hidden length after the arguments for each
 * character argument.  Handles (Vec, Mat, IS, VecScatter) are 8-byte integers
 * holding a pointer.  PetscInt is 4 bytes, PetscScalar a double.
 *
 * What belongs to this file and not to PETSc is the order of the sums inside
 * the matrix products.  They are written as SeqAIJ's loops:
 *   MatMult          y[i] = 0, then += a[i][j] x[j] over the row's entries, j ascending
 *   MatMultAdd       the same starting from the addend's y[i]
 *   MatMultTranspose y = 0, then for i ascending: y[j] += a[i][j] x[i] over the row
 * A matrix keeps every entry that was set (explicit zeros included), sorted by
 * column within its row.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef struct {
  int64_t n;
  double *a;
} svec;

typedef struct {
  int64_t nrow, ncol;
  double *val;        /* [nrow][ncol] */
  unsigned char *set; /* entry present */
} smat;

static svec *V(const int64_t *h) { return (svec *)(intptr_t)*h; }
static smat *M(const int64_t *h) { return (smat *)(intptr_t)*h; }

static void die(const char *what) {
  fprintf(stderr, "petsc_standin: %s\n", what);
  abort();
}

/* ---- Vec ---- */
void veccreate_(const int32_t *comm, int64_t *v, int32_t *ierr) {
  (void)comm;
  *v = (int64_t)(intptr_t)calloc(1, sizeof(svec));
  *ierr = 0;
}

void vecsetsizes_(int64_t *v, const int32_t *nlocal, const int32_t *n, int32_t *ierr) {
  (void)nlocal;
  svec *s = V(v);
  s->n = *n;
  s->a = (double *)calloc((size_t)(*n > 0 ? *n : 1), sizeof(double));
  if (!s->a) die("out of memory");
  *ierr = 0;
}

void vecsetfromoptions_(int64_t *v, int32_t *ierr) { (void)v; *ierr = 0; }

void vecduplicate_(const int64_t *v, int64_t *out, int32_t *ierr) {
  svec *s = (svec *)calloc(1, sizeof(svec));
  s->n = V(v)->n;
  s->a = (double *)calloc((size_t)(s->n > 0 ? s->n : 1), sizeof(double));
  if (!s->a) die("out of memory");
  *out = (int64_t)(intptr_t)s;
  *ierr = 0;
}

void vecdestroy_(int64_t *v, int32_t *ierr) {
  svec *s = V(v);
  if (s) {
    free(s->a);
    free(s);
  }
  *v = 0;
  *ierr = 0;
}

void vecgetownershiprange_(const int64_t *v, int32_t *low, int32_t *high, int32_t *ierr) {
  *low = 0;
  *high = (int32_t)V(v)->n;
  *ierr = 0;
}

void vecsetvalues_(int64_t *v, const int32_t *n, const int32_t *idx, const double *val, const int32_t *mode,
                   int32_t *ierr) {
  svec *s = V(v);
  for (int32_t i = 0; i < *n; i++) {
    if (idx[i] < 0 || idx[i] >= s->n) die("VecSetValues: index out of range");
    if (*mode == 2) s->a[idx[i]] += val[i];
    else s->a[idx[i]] = val[i];
  }
  *ierr = 0;
}

void vecassemblybegin_(int64_t *v, int32_t *ierr) { (void)v; *ierr = 0; }
void vecassemblyend_(int64_t *v, int32_t *ierr) { (void)v; *ierr = 0; }

void vecset_(int64_t *v, const double *alpha, int32_t *ierr) {
  svec *s = V(v);
  for (int64_t i = 0; i < s->n; i++) s->a[i] = *alpha;
  *ierr = 0;
}

void veccopy_(const int64_t *x, int64_t *y, int32_t *ierr) {
  if (V(x)->n != V(y)->n) die("VecCopy: sizes differ");
  memmove(V(y)->a, V(x)->a, (size_t)V(x)->n * sizeof(double));
  *ierr = 0;
}

void vecaxpy_(int64_t *y, const double *alpha, const int64_t *x, int32_t *ierr) {
  svec *sy = V(y), *sx = V(x);
  if (sx->n != sy->n) die("VecAXPY: sizes differ");
  for (int64_t i = 0; i < sy->n; i++) sy->a[i] = sy->a[i] + *alpha * sx->a[i];
  *ierr = 0;
}

void vecscale_(int64_t *v, const double *alpha, int32_t *ierr) {
  svec *s = V(v);
  for (int64_t i = 0; i < s->n; i++) s->a[i] = s->a[i] * *alpha;
  *ierr = 0;
}

void vecpointwisemult_(int64_t *w, const int64_t *x, const int64_t *y, int32_t *ierr) {
  svec *sw = V(w), *sx = V(x), *sy = V(y);
  if (sx->n != sw->n || sy->n != sw->n) die("VecPointwiseMult: sizes differ");
  for (int64_t i = 0; i < sw->n; i++) sw->a[i] = sx->a[i] * sy->a[i];
  *ierr = 0;
}

void vecview_(const int64_t *v, const int64_t *viewer, int32_t *ierr) {
  (void)viewer;
  for (int64_t i = 0; i < V(v)->n; i++) printf("%.17g\n", V(v)->a[i]);
  *ierr = 0;
}

/* for VecGetArrayF90 (petsc_standin_f90.F90) */
void standin_vec_raw_(const int64_t *v, double **a, int64_t *n) {
  *a = V(v)->a;
  *n = V(v)->n;
}

/* ---- Mat ---- */
void matcreate_(const int32_t *comm, int64_t *m, int32_t *ierr) {
  (void)comm;
  *m = (int64_t)(intptr_t)calloc(1, sizeof(smat));
  *ierr = 0;
}

void matsettype_(int64_t *m, const char *type, int32_t *ierr, size_t len) {
  (void)m;
  if (len < 3 || strncmp(type, "aij", 3) != 0) die("MatSetType: only aij");
  *ierr = 0;
}

void matsetsizes_(int64_t *m, const int32_t *mloc, const int32_t *nloc, const int32_t *nrow, const int32_t *ncol,
                  int32_t *ierr) {
  (void)mloc;
  (void)nloc;
  M(m)->nrow = *nrow;
  M(m)->ncol = *ncol;
  *ierr = 0;
}

void matsetup_(int64_t *m, int32_t *ierr) {
  smat *a = M(m);
  if (a->nrow * a->ncol > ((int64_t)1 << 27)) die("MatSetUp: the marker shape matrices (iptclshape 1, 2) are out of scope");
  size_t n = (size_t)(a->nrow * a->ncol > 0 ? a->nrow * a->ncol : 1);
  a->val = (double *)calloc(n, sizeof(double));
  a->set = (unsigned char *)calloc(n, 1);
  if (!a->val || !a->set) die("out of memory");
  *ierr = 0;
}

void matsetfromoptions_(int64_t *m, int32_t *ierr) { (void)m; *ierr = 0; }

void matsetvalues_(int64_t *m, const int32_t *nr, const int32_t *rows, const int32_t *nc, const int32_t *cols,
                   const double *val, const int32_t *mode, int32_t *ierr) {
  smat *a = M(m);
  for (int32_t i = 0; i < *nr; i++)
    for (int32_t j = 0; j < *nc; j++) {
      if (rows[i] < 0 || rows[i] >= a->nrow || cols[j] < 0 || cols[j] >= a->ncol) die("MatSetValues: index out of range");
      int64_t k = (int64_t)rows[i] * a->ncol + cols[j];
      if (*mode == 2) a->val[k] += val[(int64_t)i * *nc + j];
      else a->val[k] = val[(int64_t)i * *nc + j];
      a->set[k] = 1;
    }
  *ierr = 0;
}

void matassemblybegin_(int64_t *m, const int32_t *type, int32_t *ierr) { (void)m; (void)type; *ierr = 0; }
void matassemblyend_(int64_t *m, const int32_t *type, int32_t *ierr) { (void)m; (void)type; *ierr = 0; }

void matzeroentries_(int64_t *m, int32_t *ierr) {
  smat *a = M(m);
  memset(a->val, 0, (size_t)(a->nrow * a->ncol) * sizeof(double));
  *ierr = 0;
}

void matdestroy_(int64_t *m, int32_t *ierr) {
  smat *a = M(m);
  if (a) {
    free(a->val);
    free(a->set);
    free(a);
  }
  *m = 0;
  *ierr = 0;
}

static void mult(const smat *a, const double *x, const double *add, double *y) {
  for (int64_t i = 0; i < a->nrow; i++) {
    double sum = add ? add[i] : 0.0;
    for (int64_t j = 0; j < a->ncol; j++)
      if (a->set[i * a->ncol + j]) sum += a->val[i * a->ncol + j] * x[j];
    y[i] = sum;
  }
}

void matmult_(const int64_t *m, const int64_t *x, int64_t *y, int32_t *ierr) {
  if (V(x)->n != M(m)->ncol || V(y)->n != M(m)->nrow) die("MatMult: sizes differ");
  mult(M(m), V(x)->a, NULL, V(y)->a);
  *ierr = 0;
}

void matmultadd_(const int64_t *m, const int64_t *x, const int64_t *add, int64_t *y, int32_t *ierr) {
  if (V(x)->n != M(m)->ncol || V(y)->n != M(m)->nrow || V(add)->n != M(m)->nrow) die("MatMultAdd: sizes differ");
  mult(M(m), V(x)->a, V(add)->a, V(y)->a);
  *ierr = 0;
}

void matmulttranspose_(const int64_t *m, const int64_t *x, int64_t *y, int32_t *ierr) {
  const smat *a = M(m);
  if (V(x)->n != a->nrow || V(y)->n != a->ncol) die("MatMultTranspose: sizes differ");
  double *yy = V(y)->a;
  const double *xx = V(x)->a;
  for (int64_t j = 0; j < a->ncol; j++) yy[j] = 0.0;
  for (int64_t i = 0; i < a->nrow; i++) {
    const double alpha = xx[i];
    for (int64_t j = 0; j < a->ncol; j++)
      if (a->set[i * a->ncol + j]) yy[j] += alpha * a->val[i * a->ncol + j];
  }
  *ierr = 0;
}

/* ---- IS, VecScatter: the identity on one rank ---- */
void iscreatestride_(const int32_t *comm, const int32_t *n, const int32_t *first, const int32_t *step, int64_t *is,
                     int32_t *ierr) {
  (void)comm;
  if (*first != 0 || *step != 1) die("ISCreateStride: only the identity");
  *is = *n;
  *ierr = 0;
}

void isdestroy_(int64_t *is, int32_t *ierr) { *is = 0; *ierr = 0; }

void vecscattercreate_(const int64_t *x, const int64_t *isx, const int64_t *y, const int64_t *isy, int64_t *vs,
                       int32_t *ierr) {
  if (*isx != V(x)->n || *isy != V(y)->n || *isx != *isy) die("VecScatterCreate: only the identity");
  *vs = *isx;
  *ierr = 0;
}

void vecscatterbegin_(const int64_t *vs, const int64_t *x, int64_t *y, const int32_t *mode, const int32_t *dir,
                      int32_t *ierr) {
  (void)mode;
  (void)dir;
  if (*vs != V(x)->n || *vs != V(y)->n) die("VecScatterBegin: sizes differ");
  memmove(V(y)->a, V(x)->a, (size_t)V(x)->n * sizeof(double));
  *ierr = 0;
}

void vecscatterend_(const int64_t *vs, const int64_t *x, int64_t *y, const int32_t *mode, const int32_t *dir,
                    int32_t *ierr) {
  (void)vs; (void)x; (void)y; (void)mode; (void)dir;
  *ierr = 0;
}

void vecscatterdestroy_(int64_t *vs, int32_t *ierr) { *vs = 0; *ierr = 0; }

/* ---- MPI on one rank, printing ---- */
void mpi_allreduce_(const void *send, void *recv, const int32_t *count, const int32_t *type, const int32_t *op,
                    const int32_t *comm, int32_t *ierr) {
  (void)op;
  (void)comm;
  if (*type != 8) die("MPI_Allreduce: only MPIU_SCALAR");
  memmove(recv, send, (size_t)*count * sizeof(double));
  *ierr = 0;
}

double mpi_wtime_(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

void petscprintf_(const int32_t *comm, const char *s, int32_t *ierr, size_t len) {
  (void)comm;
  for (size_t i = 0; i < len; i++) {
    if (s[i] == '\\' && i + 1 < len && s[i + 1] == 'n') {
      fputc('\n', stdout);
      i++;
    } else {
      fputc(s[i], stdout);
    }
  }
  *ierr = 0;
}
