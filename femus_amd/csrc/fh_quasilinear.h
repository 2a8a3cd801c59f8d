// What the two element bodies that run a fh_quasilinear_form_t share (fh_quasilinear.hip: the stationary form; fh_transient.hip: one theta-step of it): the
// order of the programs, their directory in the kernel arguments, and the host step that checks a form and lays its programs back to back.
#pragma once
#include "fh_generic.h"

enum { QF_F = 0, QF_A, QF_AU, QF_C, QF_CU, QF_CG, QF_NPROG = QF_CG + 3 };

struct GenFormDir {
  int code[QF_NPROG], ncode[QF_NPROG], kons[QF_NPROG];     // first word, words (-1: no such program), first constant
};

// every refusal a form can earn on this object (c_g beyond the dimension, a program over more than max_vars variables: `vars` names them in the message), then
// all constants and all code of its programs back to back with their directory.  Nothing is enqueued and nothing of the object changes
int qf_gather_programs(const char* who, fh_generic_assembler_t as, const fh_quasilinear_form_t* form, int max_vars, const char* vars, GenFormDir& dir,
                       std::vector<int>& code, std::vector<double>& consts);
