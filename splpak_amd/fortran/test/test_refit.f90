!> `refit` of the Fortran drop-in: new values on the points of the last `initialize`.  The data are parity case "2d16" of
!! tests/cases.py (2-D, 16x16 nodes, 10^4 weighted points of the seeded Park-Miller stream, xtrap = 1) with a second
!! field y2 = cos(3 (x1 + x2)) + 0.25 y on the same points.
!!
!!   test_refit        (GPU) refit of y2 after a fit of y against a fit of y2: both lie within 1e-10 of the same minimiser,
!!                     so 2e-10 apart at most; two fields in one call; the diagnostics of the last field; and the
!!                     refusals: an object that never fitted, an object whose fit another fit of the process replaced,
!!                     set_gpus(2), nfields = 0.
!!   test_refit host   (no GPU needed) under set_host(.true.) `refit` refuses with -4 and a message instead of taking
!!                     another path; so does an object that never fitted.
program test_refit
    use splpak_module, wp => splpak_wp
    implicit none
    integer,parameter :: m = 10000, ncol = 256
    integer :: nodes(2), ierror, i, nrows, ncons, nrows2, ncons2, nbad
    real(wp) :: xdata(2,m), ydata(m), y2(m), yboth(m,2), wdata(m), xmin(2), xmax(2)
    real(wp) :: coef(ncol), coef2(ncol), cre(ncol), cboth(ncol,2), work(ncol*(ncol+1)), u(4), reserr, reserr2, omega, err
    character(len=16) :: arg
    logical :: host
    integer(8) :: s
    type(splpak_type) :: solver, other, fresh

    nbad = 0
    host = .false.
    if (command_argument_count() >= 1) then
        call get_command_argument(1, arg)
        host = trim(arg) == 'host'
    end if
    s = 42_8
    do i = 1, m
        call draw(u(1)); call draw(u(2)); call draw(u(3)); call draw(u(4))
        xdata(1,i) = u(1)
        xdata(2,i) = u(2)
        ydata(i) = sin(3.0_wp*u(1) + 1.0_wp) + sin(3.0_wp*u(2) + 2.0_wp) + 0.01_wp*(u(3) - 0.5_wp)
        wdata(i) = 0.5_wp + u(4)
        y2(i) = cos(3.0_wp*(u(1) + u(2))) + 0.25_wp*ydata(i)
    end do
    xmin = 0.0_wp; xmax = 1.0_wp; nodes = [16,16]

    ! an object that never fitted has nothing to refit
    call fresh%refit(y2,cre,ierror)
    if (ierror /= -4) call fail('refit before any initialize is not -4')

    if (host) then
        call solver%set_host(.true.)
        call solver%initialize(2,xdata,2,ydata,wdata,m,xmin,xmax,nodes,1.0_wp,coef,ncol,work,size(work),ierror)
        if (ierror /= 0) error stop 'host fit failed'
        call solver%refit(y2,cre,ierror)
        if (ierror /= -4) call fail('refit under set_host is not -4')
        if (nbad /= 0) error stop 'test_refit FAILED'
        write(*,*) 'PASS test_refit'
        stop
    end if

    ! the second field by a fit of its own, then the first field: the fit the refits continue from
    call solver%initialize(2,xdata,2,y2,wdata,m,xmin,xmax,nodes,1.0_wp,coef2,ncol,work,size(work),ierror)
    if (ierror /= 0) error stop 'fit of the second field failed'
    call solver%last_fit_info(reserr=reserr2, ndata_rows=nrows2, nconstraint_rows=ncons2)
    call solver%initialize(2,xdata,2,ydata,wdata,m,xmin,xmax,nodes,1.0_wp,coef,ncol,work,size(work),ierror)
    if (ierror /= 0) error stop 'fit failed'

    call solver%refit(y2,cre,ierror)
    if (ierror /= 0) error stop 'refit failed'
    err = maxval(abs(cre - coef2))/maxval(abs(coef2))
    write(*,'(A,ES12.3)') ' refit vs fit of the second field: ', err
    if (.not. (err < 2.0e-10_wp)) call fail('refit differs from the fit of the same values')
    call solver%last_fit_info(reserr=reserr, ndata_rows=nrows, nconstraint_rows=ncons, optimality=omega)
    write(*,'(A,I8,I8,ES12.3,ES24.16)') ' rows, constraint rows, optimality, reserr = ', nrows, ncons, omega, reserr
    if (nrows /= nrows2 .or. ncons /= ncons2) call fail('row counts of the refit')
    if (.not. (omega < 1.0e-9_wp)) call fail('optimality residual of the refit')
    if (.not. (abs(reserr - reserr2) <= 1.0e-9_wp*reserr2)) call fail('reserr of the refit')

    ! two fields in one call
    yboth(:,1) = ydata
    yboth(:,2) = y2
    call solver%refit(yboth,cboth,ierror,nfields=2)
    if (ierror /= 0) error stop 'refit of two fields failed'
    err = maxval(abs(cboth(:,1) - coef))/maxval(abs(coef))
    write(*,'(A,ES12.3)') ' field 1 of 2 vs the fit: ', err
    if (.not. (err < 2.0e-10_wp)) call fail('field 1 of 2')
    if (any(cboth(:,2) /= cre)) call fail('field 2 of 2 is not the bits of its single-field refit')

    call solver%refit(yboth,cboth,ierror,nfields=0)
    if (ierror /= -3) call fail('nfields = 0 is not -3')
    call solver%set_gpus(2)
    call solver%refit(y2,cre,ierror)
    if (ierror /= -4) call fail('refit under set_gpus(2) is not -4')
    call solver%set_gpus(1)
    call solver%refit(y2,cre,ierror)
    if (ierror /= 0) call fail('refit after the refused calls')

    ! another fit of the process replaces what the library holds: the first object's fit is no longer resident
    nodes = [12,12]
    call other%initialize(2,xdata,2,ydata,wdata,m,xmin,xmax,nodes,1.0_wp,coef,ncol,work,size(work),ierror)
    if (ierror /= 0) error stop 'fit of another grid failed'
    call solver%refit(y2,cre,ierror)
    if (ierror /= -4) call fail('refit of a fit that is no longer resident is not -4')
    call other%refit(y2,cre,ierror)
    if (ierror /= 0) call fail('refit of the resident fit')

    call solver%destroy()
    if (nbad /= 0) error stop 'test_refit FAILED'
    write(*,*) 'PASS test_refit'
contains
    subroutine draw(v)
        real(wp),intent(out) :: v
        s = mod(48271_8*s, 2147483647_8)
        v = real(real(s,8)/2147483647.0_8, wp)
    end subroutine draw
    subroutine fail(what)
        character(len=*),intent(in) :: what
        write(*,*) 'FAILED: ', what
        nbad = nbad + 1
    end subroutine fail
end program test_refit
